"""The LoRA reference ops (ops/ref.py) — the rounding contract the HIP
kernels are held to: f32 shrink result and delta, one rounding at the
final add, slice-table semantics, no-adapter rows untouched."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.ops import ref

from lora_cases import (RANK_CASES, SHAPES, bf16_ulp_distance, random_case,
                        ref_out, shuffled_ref_out)

BF16 = torch.bfloat16


def make(T, K, O, r, n_adapters, seed, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((T, K), generator=g).to(dtype)
    A = (torch.randn((n_adapters, r, K), generator=g) / K ** 0.5).to(dtype)
    B = (torch.randn((n_adapters, O, r), generator=g) / r ** 0.5).to(dtype)
    out = torch.randn((T, O), generator=g).to(dtype)
    scale = torch.tensor([0.5, 2.0, 1.25][:n_adapters], dtype=torch.float32)
    return x, A, B, out, scale


def test_matches_direct_f32_composition():
    x, A, B, out, scale = make(7, 96, 40, 8, 3, seed=1)
    idx = torch.tensor([0, 1, 2, 2, 1, 0, 1], dtype=torch.int32)
    y = ref.lora_shrink(x, A, idx)
    assert y.dtype == torch.float32 and y.shape == (7, 8)
    got = ref.lora_expand_add_(out.clone(), y, B, scale, [40], idx)
    for t in range(7):
        a = int(idx[t])
        want_y = x[t].float() @ A[a].float().t()
        torch.testing.assert_close(y[t], want_y, rtol=1e-5, atol=1e-5)
        delta = x[t].float() @ A[a].float().t() @ B[a].float().t()
        want = (out[t].float() + scale[a] * delta).to(BF16)
        # one rounding: at most the neighbouring bf16 value apart from a
        # composition whose f32 sums ran in another order
        assert int(bf16_ulp_distance(got[t], want).max()) <= 1
    assert got.dtype == BF16


def test_cpu_wrappers_fall_back_to_the_reference():
    x, A, B, out, scale = make(5, 64, 24, 4, 2, seed=2)
    idx = torch.tensor([1, -1, 0, 0, 1], dtype=torch.int32)
    y = ops.lora_shrink(x, A, idx)
    assert torch.equal(y, ref.lora_shrink(x, A, idx))
    a = ops.lora_expand_add_(out.clone(), y, B, scale, [24], idx)
    b = ref.lora_expand_add_(out.clone(), y, B, scale, [24], idx)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_three_unequal_slices():
    """Output row o of slice s reads ranks [s*r, (s+1)*r) of the shrink
    result: a fused q|k|v projection equals three separate adapters."""
    T, K, r = 6, 48, 4
    widths = [20, 7, 13]
    O = sum(widths)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((T, K), generator=g).to(BF16)
    As = [torch.randn((2, r, K), generator=g).to(BF16) for _ in widths]
    Bs = [torch.randn((2, w, r), generator=g).to(BF16) for w in widths]
    out = torch.randn((T, O), generator=g).to(BF16)
    scale = torch.tensor([0.5, 2.0])
    idx = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32)
    A = torch.cat(As, dim=1)                       # [2, 3r, K]
    B = torch.cat(Bs, dim=1)                       # [2, O, r]
    got = ref.lora_expand_add_(out.clone(), ref.lora_shrink(x, A, idx), B,
                               scale, [20, 27, 40], idx)
    lo = 0
    for As_s, Bs_s, w in zip(As, Bs, widths):
        part = out[:, lo:lo + w].clone()
        ref.lora_expand_add_(part, ref.lora_shrink(x, As_s, idx), Bs_s, scale,
                             [w], idx)
        assert torch.equal(got[:, lo:lo + w].view(torch.int16),
                           part.contiguous().view(torch.int16))
        lo += w
    # a wrong slice would have read another A: the slices really differ
    wrong = ref.lora_expand_add_(out.clone(), ref.lora_shrink(x, A, idx), B,
                                 scale, [7, 27, 40], idx)
    assert not torch.equal(wrong, got)
    for bad in ([20, 27], [27, 20, 40], [0, 20, 40], [10, 20, 30, 40]):
        with pytest.raises(ValueError):
            ref.lora_expand_add_(out.clone(), ref.lora_shrink(x, A, idx), B,
                                 scale, bad, idx)


def test_rows_without_adapter_are_bit_unchanged():
    x, A, B, out, scale = make(9, 64, 32, 8, 2, seed=4)
    out[1, 3] = float("nan")                        # survives as the same bits
    idx = torch.tensor([0, -1, 1, -1, -1, 0, 1, -1, 0], dtype=torch.int32)
    y = ref.lora_shrink(x, A, idx)
    got = ref.lora_expand_add_(out.clone(), y, B, scale, [32], idx)
    none = idx < 0
    assert torch.equal(got[none].view(torch.int16),
                       out[none].view(torch.int16))
    assert not torch.equal(got[~none], out[~none])
    assert float(y[none].abs().max()) == 0.0
    # every row -1: nothing happens at all
    all_none = torch.full((9,), -1, dtype=torch.int32)
    got = ref.lora_expand_add_(out.clone(), ref.lora_shrink(x, A, all_none),
                               B, scale, [32], all_none)
    assert torch.equal(got.view(torch.int16), out.view(torch.int16))


def test_rank_below_r_max_equals_its_zero_padded_form():
    T, K, O, r, r_max = 5, 80, 24, 3, 8
    x, A, B, out, scale = make(T, K, O, r, 2, seed=5)
    idx = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32)
    small = ref.lora_expand_add_(out.clone(), ref.lora_shrink(x, A, idx), B,
                                 scale, [O], idx)
    Ap = torch.zeros((2, r_max, K), dtype=BF16)
    Bp = torch.zeros((2, O, r_max), dtype=BF16)
    Ap[:, :r] = A
    Bp[:, :, :r] = B
    padded = ref.lora_expand_add_(out.clone(), ref.lora_shrink(x, Ap, idx),
                                  Bp, scale, [O], idx)
    assert torch.equal(small.view(torch.int16), padded.view(torch.int16))


@pytest.mark.parametrize("r_max,n_slices", RANK_CASES)
def test_reference_order_sensitivity_stays_under_the_cap(r_max, n_slices):
    """The device test allows the kernel 1 bf16 ulp and < 1 % differing
    elements against this reference, since both round once from f32 sums
    that differ only in order.  Here the reference itself, evaluated in a
    shuffled summation order on the device test's own data and seeds,
    must stay inside that allowance — otherwise the cap would be about
    the data, not the kernel."""
    worst, worst_frac = 0, 0.0
    for T, K, O in SHAPES:
        if T == 65:                 # the 3- and 257-row shapes bracket it
            continue
        case = random_case(T, K, O, r_max, n_slices)
        d = bf16_ulp_distance(ref_out(case)[1], shuffled_ref_out(case))
        worst = max(worst, int(d.max()))
        worst_frac = max(worst_frac, float((d != 0).float().mean()))
    assert worst <= 1, worst
    assert worst_frac < 0.01, worst_frac
