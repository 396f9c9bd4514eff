"""SwiGLU fused into the int4 down projection (ops.w4a16_silu_linear and
its zero-point form) on the device: bit equality with ops.silu_mul followed
by the plain op, the float64 oracle under the plain op's bound
(tests/test_w4a16_gpu.py), the argument checks and the model routing."""

import functools

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import PagedKVCache
from resilient_llm_amd.models import LlamaForCausalLM, get_config

import awq_cases
import w4a16_cases
from w4a16_cases import BF16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (N, K, splitk): one group, several, a K the default plan (0) slices;
# splitk forced to 1 and, where K has groups to cut, to 3
NKS = [(N, K, sk) for N, K in [(64, 128), (128, 512), (64, 2048)]
       for sk in (0, 1, 3) if sk <= 1 or K >= 256]
# (fused op, plain op) per form
OPS = {"sym": (ops.w4a16_silu_linear, ops.w4a16_linear),
       "zp": (ops.w4a16_zp_silu_linear, ops.w4a16_zp_linear)}


@functools.lru_cache(maxsize=None)
def weights(form, N, K):
    """(random case, packed, s or meta on the device), shared by all M."""
    case = (w4a16_cases if form == "sym" else awq_cases).random_case(1, N, K)
    sm = case.s if form == "sym" else case.meta
    return case, case.packed.to(DEV), sm.to(DEV)


def gate_up(M, K):
    """gu [M, 2K] ~ 4 N(0, 1): the first rows of a taller tensor whose
    other rows are NaN."""
    g = torch.Generator().manual_seed(M + K)
    tall = torch.full((M + 3, 2 * K), float("nan"), dtype=BF16)
    tall[:M] = (4 * torch.randn(M, 2 * K, generator=g)).to(BF16)
    return tall.to(DEV)[:M]


@pytest.mark.parametrize("N,K,splitk", NKS)
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33, 64])
@pytest.mark.parametrize("form", ["sym", "zp"])
def test_bit_identical_to_silu_mul_then_linear(form, M, N, K, splitk):
    fused, plain = OPS[form]
    _, packed, sm = weights(form, N, K)
    gu = gate_up(M, K)
    ws = torch.full((16 * M * N,), float("nan"), device=DEV)
    got = fused(gu, packed, sm, splitk, ws=ws)
    want = plain(ops.silu_mul(gu), packed, sm, splitk)
    assert not bool(want.isnan().any())
    assert torch.equal(got, want)
    assert torch.equal(fused(gu, packed, sm, splitk, ws=ws), got)


@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (64, 64, 2048)])
@pytest.mark.parametrize("form", ["sym", "zp"])
def test_within_the_plain_ops_bound_of_the_float64_oracle(form, M, N, K):
    """a = bf16(silu(g) * u) computed in float64, then the bound of
    test_w4a16_gpu.py::test_random_bf16_within_the_bound on the GEMM:
    |got - y64| <= 2^-8 |y64| + 2^-19 S."""
    case, packed, sm = weights(form, N, K)
    gu = gate_up(M, K)
    g, u = gu.cpu().double().split(K, dim=1)
    a = (g / (1 + torch.exp(-g)) * u).to(BF16)
    mod = w4a16_cases if form == "sym" else awq_cases
    y, allowed, _ = mod.random_bound(case._replace(x=a))
    err = (OPS[form][0](gu, packed, sm).cpu().double() - y).abs()
    print(f"w4a16_silu {form} {(M, N, K)}: max err/allowed "
          f"{float((err / allowed).max()):.3f}")
    assert bool((err <= allowed).all()), float((err / allowed).max())


# (M, gu width, dtype, ws elements) against K = 256, splitk = 2
@pytest.mark.parametrize("M,width,dtype,n_ws", [
    (3, 511, BF16, None), (3, 768, BF16, None), (0, 512, BF16, None),
    (65, 512, BF16, None), (3, 512, torch.float32, None), (3, 512, BF16, 8)])
def test_argument_checks(M, width, dtype, n_ws):
    for form, (fused, _) in OPS.items():
        _, packed, sm = weights(form, 64, 256)
        ws = None if n_ws is None else torch.empty(n_ws, device=DEV)
        with pytest.raises(RuntimeError):
            fused(torch.zeros(M, width, dtype=dtype, device=DEV), packed, sm,
                  2, ws=ws)


@pytest.mark.parametrize("quant,op", [("int4", "w4a16_silu_linear"),
                                      ("int4-awq", "w4a16_zp_silu_linear")])
def test_model_routes_small_steps_to_the_fused_op(quant, op, monkeypatch):
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=3, quant=quant)
    calls, real = [], getattr(ops, op)
    monkeypatch.setattr(ops, op,
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))

    def decode(rows):
        monkeypatch.setattr(LlamaForCausalLM, "_W4_SILU_ROWS", rows)
        del calls[:]
        kv = PagedKVCache.for_model(cfg, 4, device=DEV)
        i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)
        return model.forward_decode(
            i32([5, 6, 7, 8]), i32([0] * 4), kv, i32([0, 16, 32, 48]),
            i32([[0], [1], [2], [3]]), i32([1] * 4)), len(calls)

    fused, n_fused = decode(64)
    plain, n_plain = decode(0)
    assert (n_fused, n_plain) == (cfg.n_layers, 0)
    assert not bool(fused.isnan().any()) and torch.equal(fused, plain)
