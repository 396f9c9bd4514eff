"""The AWQ int4 format on the CPU: the AutoAWQ packing against its
description, the asymmetric quantizer's error, and what the config and the
loader refuse (tests/awq_cases.py holds the
constructions)."""

import pytest
import torch

from resilient_llm_amd.config import ConfigError, load_config
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.ops import ref

from awq_cases import awq_pack, layer_case, write_awq_checkpoint


def test_anchor_dword_and_round_trip():
    row = torch.arange(8, dtype=torch.uint8).repeat(8)[None, :]   # N = 64
    u = row.t().repeat(1, 128)                                    # [64, 128]
    qw, qz, sc = awq_pack(u, u[:, :1], torch.ones(64, 1).half())
    assert int(qw[0, 0]) == 0x75316420 and int(qz[0, 3]) == 0x75316420
    for N, K in ((64, 128), (192, 384)):
        u, z, s, _ = layer_case(N, K)
        qw, qz, sc = awq_pack(u, z, s)
        assert qw.shape == (K, N // 8) and qz.shape == (K // 128, N // 8)
        assert sc.shape == (K // 128, N) and sc.dtype == torch.float16
        for got, want in zip(ref.awq_unpack(qw, qz, sc), (u, z, s)):
            assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ref.awq_unpack(qw, qz, sc.bfloat16())


def test_quantize_w4_zp_error_at_most_half_a_step():
    g = torch.Generator().manual_seed(3)
    w = (0.02 * torch.randn(64, 512, generator=g)).to(torch.bfloat16)
    w[0, :128] = w[0, :128].abs() + 1.0      # a group far from 0
    w[1, :128] = 0.0                         # an all-zero group
    u, z, s = ref.quantize_w4_zp(w)
    assert int(u.max()) <= 15 and int(z.max()) <= 15
    assert s.dtype == torch.float16 and bool((s > 0).all())
    step = s.double().repeat_interleave(128, dim=1)
    rec = step * (u.double() - z.double().repeat_interleave(128, dim=1))
    assert bool(((rec - w.double()).abs() <= step / 2).all())


def _cfg(*lps, pools=None):
    return {"cluster": {"port": 4999, **({"pools": pools} if pools else {})},
            "model_list": [{"model_name": f"m{i}", "litellm_params": lp}
                           for i, lp in enumerate(lps)]}


def test_config_accepts_awq_on_gpu_workers_only():
    cfg = load_config(data=_cfg({"model": "gpu/0/llama-3-8b",
                                 "quantization": "int4-awq", "weights": "/w"}))
    assert cfg.deployments[0].params["quantization"] == "int4-awq"
    with pytest.raises(ConfigError, match="int4-awq"):
        load_config(data=_cfg(
            {"model": "pool/p/llama-3-8b", "quantization": "int4-awq"},
            pools={"p": {"gpus": [0, 1], "tensor_parallel": 2}}))
    with pytest.raises(ConfigError, match="quantization: int4-awq"):
        load_config(data=_cfg(
            {"model": "gpu/0/llama-3-8b", "quantization": "int4-awq",
             "adapters": {"x": "/a/x"}, "adapter": "x"}))
    with pytest.raises(ValueError, match="tensor_parallel"):
        LlamaForCausalLM(get_config("tiny"), device="cpu", quant="int4-awq",
                         tp_rank=0, tp_world=2)


@pytest.mark.parametrize("field,value", [
    ("quant_method", "gptq"), ("bits", 8), ("group_size", 64),
    ("version", "gemv"), ("zero_point", False)])
def test_loader_names_the_bad_quantization_config_field(tmp_path, field,
                                                        value):
    cfg = get_config("tiny")
    dense = LlamaForCausalLM(cfg, device="cpu", seed=2)
    write_awq_checkpoint(dense, str(tmp_path), **{field: value})
    m = LlamaForCausalLM(cfg, device="cpu", seed=1, quant="int4-awq")
    with pytest.raises(ValueError, match=field):
        m.load_safetensors(str(tmp_path))


def test_dense_and_awq_weights_do_not_cross(tmp_path):
    cfg = get_config("tiny")
    dense = LlamaForCausalLM(cfg, device="cpu", seed=2)
    dense.save_safetensors(str(tmp_path / "dense"))
    write_awq_checkpoint(dense, str(tmp_path / "awq"))
    with pytest.raises(ValueError, match="dense"):
        LlamaForCausalLM(cfg, device="cpu", quant="int4-awq").load_safetensors(
            str(tmp_path / "dense"))
    for quant in (None, "int4", "fp8"):
        with pytest.raises(ValueError, match="AWQ"):
            LlamaForCausalLM(cfg, device="cpu", quant=quant).load_safetensors(
                str(tmp_path / "awq"))
