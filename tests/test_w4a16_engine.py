"""``quant="int4"`` through the model, the engine, the config and the
worker CLI on the CPU (the fused op runs as its reference there)."""

import asyncio
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from resilient_llm_amd.config import ConfigError, load_config
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.ops import ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJS = ("qkv", "o", "gate_up", "down")


def drain(engine, max_steps=1000):
    outs = {}
    for _ in range(max_steps):
        if not engine.has_work():
            break
        for o in engine.step():
            outs.setdefault(o.req_id, []).append(o.token_id)
    assert not engine.has_work()
    return outs


def test_int4_params_and_exact_param_bytes():
    cfg = get_config("tiny-128")
    dense = LlamaForCausalLM(cfg, device="cpu", seed=4)
    quant = LlamaForCausalLM(cfg, device="cpu", seed=4, quant="int4")
    expected = dense.param_bytes()
    for i in range(cfg.n_layers):
        for n in PROJS:
            name = f"l{i}.{n}"
            N, K = dense.params[name].shape
            assert name not in quant.params
            q4, s4 = quant.params[name + ".q4"], quant.params[name + ".s4"]
            assert q4.dtype == torch.int32 and q4.numel() == N * K // 8
            assert s4.dtype == torch.bfloat16
            assert tuple(s4.shape) == (N, K // 128)
            # the stored weight IS the quantized dense one
            q, s = ref.quantize_w4(dense.params[name])
            assert torch.equal(ref.w4_unpack(q4, N, K), q)
            assert torch.equal(s4, s)
            expected += N * K // 2 + N * K // 128 * 2 - N * K * 2
    # everything else is untouched bf16
    for name in ("embed", "lm_head", "final_ln", "l0.ln1", "l1.ln2"):
        assert quant.params[name].dtype == torch.bfloat16
        assert torch.equal(quant.params[name], dense.params[name])
    assert set(quant.params) == (
        {k for k in dense.params if k.split(".")[-1] not in PROJS}
        | {f"l{i}.{n}{sfx}" for i in range(cfg.n_layers) for n in PROJS
           for sfx in (".q4", ".s4")})
    assert quant.param_bytes() == expected
    assert quant.param_bytes() < 0.5 * dense.param_bytes()


def test_int4_rejects_unknown_quant_and_refuses_save_and_adapters(tmp_path):
    cfg = get_config("tiny")
    with pytest.raises(ValueError):
        LlamaForCausalLM(cfg, device="cpu", quant="awq")
    m = LlamaForCausalLM(cfg, device="cpu", quant="int4")
    with pytest.raises(RuntimeError):
        m.save_safetensors(str(tmp_path / "w"))
    with pytest.raises(RuntimeError, match="quantized"):
        m.add_adapter("a", 4, 8.0, ["q_proj"], {})


def test_int4_quantizes_again_after_a_safetensors_load(tmp_path):
    cfg = get_config("tiny")
    src = LlamaForCausalLM(cfg, device="cpu", seed=9)
    src.save_safetensors(str(tmp_path / "w"))
    m = LlamaForCausalLM(cfg, device="cpu", seed=1, quant="int4")
    m.load_safetensors(str(tmp_path / "w"))
    for n in PROJS:
        assert f"l0.{n}" not in m.params
        N, K = src.params[f"l0.{n}"].shape
        q, s = ref.quantize_w4(src.params[f"l0.{n}"])
        assert torch.equal(ref.w4_unpack(m.params[f"l0.{n}.q4"], N, K), q)
        assert torch.equal(m.params[f"l0.{n}.s4"], s)


def test_int4_tensor_parallel_shards_quantize_per_rank():
    """Each rank quantizes its own shard: groups run along the rank's K."""
    cfg = get_config("tiny")
    full = LlamaForCausalLM(cfg, device="cpu", seed=2)
    for rank in (0, 1):
        dense = LlamaForCausalLM(cfg, device="cpu", seed=2, tp_rank=rank,
                                 tp_world=2)
        quant = LlamaForCausalLM(cfg, device="cpu", seed=2, tp_rank=rank,
                                 tp_world=2, quant="int4")
        for n in PROJS:
            w = dense.params[f"l1.{n}"]
            N, K = w.shape
            q, s = ref.quantize_w4(w)
            assert torch.equal(
                ref.w4_unpack(quant.params[f"l1.{n}.q4"], N, K), q)
            assert torch.equal(quant.params[f"l1.{n}.s4"], s)
        assert dense.params["l1.down"].shape[1] * 2 \
            == full.params["l1.down"].shape[1]


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
def test_int4_engine_completes_a_generation(model_name):
    cfg = get_config(model_name)
    m = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=3,
                         quant="int4")
    e = LLMEngine(m, PagedKVCache.for_model(cfg, 64, device="cpu"),
                  max_batch_size=4)
    for i in range(3):
        e.add_request(f"r{i}", list(range(5 + i, 30 + 2 * i)),
                      SamplingParams(max_tokens=6))
    outs = drain(e)
    assert sorted(outs) == ["r0", "r1", "r2"]
    assert all(len(v) == 6 for v in outs.values())


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
@pytest.mark.parametrize("seed", [4, 5, 6])
def test_int4_prefill_logits_cosine_to_dense(model_name, seed):
    """Round-to-nearest int4 keeps the prefill logits of the 32-token
    prompt within cosine 0.93 of the dense model (measured 0.955-0.978):
    room for rounding-mode details, none for a wrong group or scale."""
    cfg = get_config(model_name)
    dense = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32,
                             seed=seed)
    quant = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32,
                             seed=seed, quant="int4")
    ids = torch.arange(5, 37, dtype=torch.int32)
    pos = torch.arange(32, dtype=torch.int32)
    cu = torch.tensor([0, 32], dtype=torch.int32)

    def logits(m):
        kv = PagedKVCache.for_model(cfg, 32)
        blocks = kv.allocate(3)
        slot = torch.tensor([blocks[p // 16] * 16 + p % 16
                             for p in range(32)], dtype=torch.int32)
        return m.forward_prefill(ids, pos, kv, slot, cu).float()
    ld, lq = logits(dense), logits(quant)
    cos = float(F.cosine_similarity(ld.flatten(), lq.flatten(), dim=0))
    print(f"{model_name} seed {seed}: cosine {cos:.4f}")
    assert cos >= 0.93, cos
    # a wrong scale group does not pass: shift every scale by one group
    s4 = quant.params["l0.gate_up.s4"]
    quant.params["l0.gate_up.s4"] = torch.roll(s4, 1, dims=1) * 4
    bad = float(F.cosine_similarity(ld.flatten(), logits(quant).flatten(),
                                    dim=0))
    assert bad < cos


def _cfg(model_list):
    return {"cluster": {"port": 4999}, "model_list": model_list}


def test_config_accepts_int4_and_keeps_the_other_errors():
    def one(**lp):
        return _cfg([{"model_name": "m", "litellm_params": {
            "model": "gpu/0/llama-3-8b", **lp}}])
    cfg = load_config(data=one(quantization="int4"))
    assert cfg.deployments[0].params["quantization"] == "int4"
    load_config(data=one(quantization="int4", kv_dtype="fp8"))
    for bad in (one(kv_dtype="int4"), one(quantization="awq"),
                one(quantization="int8"), one(quantization=4)):
        with pytest.raises(ConfigError):
            load_config(data=bad)


def test_config_rejects_adapters_with_int4_weights():
    with pytest.raises(ConfigError, match="quantization: int4"):
        load_config(data=_cfg([
            {"model_name": "a", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "quantization": "int4",
                "adapters": {"x": "/a/x"}, "adapter": "x"}}]))
    with pytest.raises(ConfigError, match="quantization"):
        load_config(data=_cfg([
            {"model_name": "a", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "quantization": "int4"}},
            {"model_name": "b", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "adapters": {"x": "/a/x"}}}]))
    # another worker's quantization does not count
    load_config(data=_cfg([
        {"model_name": "a", "litellm_params": {
            "model": "gpu/0/llama-3-8b", "quantization": "int4"}},
        {"model_name": "b", "litellm_params": {
            "model": "gpu/1/llama-3-8b", "adapters": {"x": "/a/x"}}}]))


def test_gpu_main_quant_int4_serves_a_request():
    """``gpu_main --quant int4`` parses and the worker it starts answers
    (on the CPU device the tests use)."""
    from resilient_llm_amd.workers.base import GenerationRequest
    from resilient_llm_amd.workers.rpc import RpcWorkerClient
    sock = os.path.join(tempfile.mkdtemp(prefix="rlli-test-"), "w.sock")
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.Popen(
        [sys.executable, "-m", "resilient_llm_amd.workers.gpu_main",
         "--device-label", "gpu:9", "--model", "tiny", "--socket", sock,
         "--device", "cpu", "--num-blocks", "64", "--quant", "int4"],
        env=env)

    async def run():
        client = RpcWorkerClient("gpu:9", {"tiny"}, sock)
        client.proc = proc
        await client.connect(timeout=60)
        res = await client.generate(GenerationRequest(
            request_id="q1", model="tiny",
            messages=[{"role": "user", "content": "hello int4"}],
            max_tokens=5))
        assert res.completion_tokens == 5
        await client.close()
    try:
        asyncio.run(run())
    finally:
        if proc.poll() is None:
            proc.terminate()
            proc.wait(timeout=10)
    # an unknown value is an argparse error, not a dead worker later
    r = subprocess.run(
        [sys.executable, "-m", "resilient_llm_amd.workers.gpu_main",
         "--device-label", "gpu:9", "--model", "tiny", "--socket", sock,
         "--device", "cpu", "--quant", "awq"], env=env,
        capture_output=True, text=True)
    assert r.returncode == 2 and "--quant" in r.stderr
