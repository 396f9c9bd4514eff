"""Mixture-of-Experts on the CPU: the reference ops, the tiny-moe model's
checkpoint names, the config rules and an engine run."""

import dataclasses

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.config import MOE_MODELS, ConfigError, load_config
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import (MODEL_PRESETS, LlamaForCausalLM,
                                      get_config)
from resilient_llm_amd.ops import ref


def test_ref_moe_mlp_equals_per_token_loop():
    torch.manual_seed(0)
    T, H, I, E, k = 7, 64, 64, 6, 3
    x = torch.randn(T, H).bfloat16()
    wgu = (torch.randn(E, 2 * I, H) * 0.2).bfloat16()
    wd = (torch.randn(E, H, I) * 0.2).bfloat16()
    ids, w = ops.moe_route(torch.randn(T, E).bfloat16(), k)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert torch.allclose(w.sum(-1), torch.ones(T))
    want = torch.zeros(T, H, dtype=torch.float64)
    for t in range(T):
        for j in range(k):
            e = int(ids[t, j])
            gu = wgu[e].double() @ x[t].double()
            act = torch.nn.functional.silu(gu[:I]) * gu[I:]
            want[t] += w[t, j].double() * (wd[e].double() @ act)
    got = ref.moe_mlp(x, ids, w, wgu, wd, exact=True)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # the CPU op: the same with the two bf16 roundings of the kernels
    out = ops.moe_mlp(x, ids, w, wgu, wd)
    assert out.dtype == torch.bfloat16
    assert (out.double() - want).abs().max() <= 2 ** -6 * want.abs().max()
    with pytest.raises(ValueError, match="H % 64"):
        ops.moe_mlp(x[:, :32], ids, w, wgu[:, :, :32], wd[:, :32])


def test_ref_route_ties_and_nan():
    lg = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0],
                       [float("nan"), 2.0, float("-inf"), 2.0, 5.0, 1.0]])
    ids, w = ref.moe_route(lg.bfloat16(), 4, renorm=False)
    assert ids.tolist() == [[1, 2, 5, 0], [4, 1, 3, 5]]
    assert torch.allclose(w[0], torch.softmax(lg[0], -1)[ids[0].long()])


def test_checkpoint_round_trip_and_mismatches(tmp_path):
    cfg = get_config("tiny-moe")
    m = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=4)
    path = str(tmp_path / "moe")
    m.save_safetensors(path)
    import safetensors.torch as st
    keys = set(st.load_file(path + "/model.safetensors"))
    p = "model.layers.1.mlp."
    assert {p + "gate.weight", p + "experts.7.gate_proj.weight",
            p + "experts.0.up_proj.weight",
            p + "experts.3.down_proj.weight"} <= keys
    assert p + "gate_proj.weight" not in keys
    twin = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=9)
    twin.load_safetensors(path)
    for i in range(cfg.n_layers):
        for n in ("router", "experts_gate_up", "experts_down"):
            assert torch.equal(twin.params[f"l{i}.{n}"], m.params[f"l{i}.{n}"])
    dense_cfg = dataclasses.replace(cfg, name="tiny-dense", num_experts=0)
    dense = LlamaForCausalLM(dense_cfg, device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.experts\.0\.down"):
        dense.load_safetensors(path)
    path2 = str(tmp_path / "dense")
    dense.save_safetensors(path2)
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.gate_proj"):
        twin.load_safetensors(path2)


def _cfg(model, pools=None, **params):
    return {"cluster": {"pools": pools or {}},
            "model_list": [{"model_name": "m",
                            "litellm_params": {"model": model, **params}}]}


@pytest.mark.parametrize("data, match", [
    (_cfg("gpu/0/tiny-moe", quantization="int4"), "quantization"),
    (_cfg("gpu/0/tiny-moe", adapters={"a": "/x"}), "adapters"),
    (_cfg("pool/p/qwen3-30b-a3b",
          pools={"p": {"gpus": [0, 1], "tensor_parallel": 2}}),
     "tensor_parallel"),
    (_cfg("pool/p/tiny-moe", pools={"p": {"gpus": [0]}}), "gpu/<device>"),
])
def test_config_rejects(data, match):
    with pytest.raises(ConfigError, match=match):
        load_config(data=data)


def test_config_accepts_and_lists_the_moe_presets():
    load_config(data=_cfg("gpu/0/qwen3-30b-a3b"))
    assert MOE_MODELS == {n for n, c in MODEL_PRESETS.items() if c.num_experts}
    c = get_config("qwen3-30b-a3b")
    assert (c.num_experts, c.experts_per_token, c.moe_intermediate_size,
            c.hidden_size, c.norm_topk_prob) == (128, 8, 768, 2048, True)
    with pytest.raises(ValueError, match="quant"):
        LlamaForCausalLM(get_config("tiny-moe"), quant="int4")


def test_tiny_moe_engine_generates():
    cfg = get_config("tiny-moe")
    m = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=2)
    kv = PagedKVCache.for_model(cfg, 32, device="cpu")
    kv.k, kv.v = kv.k.float(), kv.v.float()
    free0 = kv.free_blocks
    e = LLMEngine(m, kv, max_batch_size=4)
    for r in range(3):
        e.add_request(f"r{r}", list(range(3 + r, 30 + 3 * r)),
                      SamplingParams(max_tokens=6, temperature=0.0))
    n = 0
    while e.has_work():
        n += len(e.step())
    assert n == 18 and kv.free_blocks == free0
