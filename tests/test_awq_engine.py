"""``quant="int4-awq"`` through the model and the engine: GPU logits
against the CPU fp32 twin holding the same quantized weights, and a synthetic
AutoAWQ checkpoint directory loading to the tensors of the model it was
written from (on the CPU, and through the device repack on the GPU)."""

import pytest
import torch

from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config

from awq_cases import write_awq_checkpoint
from test_w4a16_gpu import _cpu_twin, _logits_pair, _rel, drain

DEV = "cuda:0"
MODELS = ["tiny", "tiny-128"]


def _twin(gpu_model, cfg):
    twin = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=0,
                            quant="int4-awq")
    for k, v in gpu_model.params.items():
        v = v.detach().cpu()
        twin.params[k] = v if k.endswith((".q4", ".m4")) else v.float()
    twin.cos_sin = gpu_model.cos_sin.cpu()
    return twin


@pytest.mark.gpu
@pytest.mark.parametrize("model_name", MODELS)
def test_awq_logits_against_cpu_fp32_twin(model_name):
    """max|err| / max|logit| of the awq GPU model against the CPU fp32
    model holding the same packed / meta tensors is at most 2x the same
    measure of the bf16 GPU model against its CPU fp32 twin, for a
    40-token prefill and one decode step of a batch of 3 (the int4 engine
    test's criterion)."""
    cfg = get_config(model_name)
    dense = LlamaForCausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=6)
    base = [_rel(g, c) for g, c in zip(
        _logits_pair(dense, cfg, DEV),
        _logits_pair(_cpu_twin(dense, cfg, None), cfg, "cpu"))]
    quant = LlamaForCausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=6,
                             quant="int4-awq")
    got = [_rel(g, c) for g, c in zip(
        _logits_pair(quant, cfg, DEV),
        _logits_pair(_twin(quant, cfg), cfg, "cpu"))]
    print(f"{model_name}: awq prefill/decode rel err {got[0]:.4e} "
          f"{got[1]:.4e}; bf16 baseline {base[0]:.4e} {base[1]:.4e}")
    for what, g, b in zip(("prefill", "decode"), got, base):
        assert g <= 2 * b, (what, g, b)


@pytest.mark.parametrize("device", [
    "cpu", pytest.param(DEV, marks=pytest.mark.gpu)])
@pytest.mark.parametrize("model_name", MODELS)
def test_synthetic_checkpoint_loads_to_the_models_tensors(model_name, device,
                                                          tmp_path):
    cfg = get_config(model_name)
    dtype = torch.float32 if device == "cpu" else torch.bfloat16
    kw = dict(device=device, dtype=dtype)
    model = LlamaForCausalLM(cfg, seed=7, quant="int4-awq", **kw)
    held = write_awq_checkpoint(LlamaForCausalLM(cfg, seed=7, **kw),
                                str(tmp_path))
    loaded = LlamaForCausalLM(cfg, seed=8, quant="int4-awq", **kw)
    n = loaded.load_safetensors(str(tmp_path))
    assert n == cfg.n_layers * (7 * 3 + 2) + 2 + (not cfg.tie_embeddings)
    assert set(loaded.params) == set(model.params)
    for name, (packed, meta) in held.items():
        for sfx, want in ((".q4", packed), (".m4", meta)):
            assert torch.equal(loaded.params[name + sfx].cpu(), want), name
            assert torch.equal(model.params[name + sfx].cpu(), want), name

    def greedy(m):
        e = LLMEngine(m, PagedKVCache.for_model(cfg, 64, device=device),
                      max_batch_size=4)
        e.add_request("a", list(range(5, 30)), SamplingParams(max_tokens=6))
        e.add_request("b", list(range(40, 47)), SamplingParams(max_tokens=6))
        return drain(e)
    out = greedy(loaded)
    assert out == greedy(model) and all(len(v) == 6 for v in out.values())
