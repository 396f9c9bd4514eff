"""The int4 group-quantized weight format on the CPU: packing round
trips, the quantizer's invariants, and the reference ops against their
definitions (tests/w4a16_cases.py holds the constructions)."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.ops import ref

from w4a16_cases import (BF16, GROUP, dequant_case, exact_case, needle_case,
                         needle_weights, oracle64, random_bound, random_case)


def test_pack_unpack_round_trip_every_value_every_position():
    """All 16 nibble values at every position of a group (and in every
    column of a 16-column tile): value (v + k + n) % 16 at (n, k)."""
    N, K = 64, 2 * GROUP
    for v in range(16):
        q = ((torch.arange(N)[:, None] + torch.arange(K)[None, :] + v) % 16
             - 8).to(torch.int8)
        packed = ref.w4_pack(q)
        assert packed.dtype == torch.int32 and packed.numel() == N * K // 8
        assert torch.equal(ref.w4_unpack(packed, N, K), q)


def test_pack_is_a_bijection_on_single_nibbles():
    """One non-zero-offset nibble at a time: each (n, k) owns its own four
    bits of ``packed`` (u = q + 8, so q = -8 is the all-zero pattern)."""
    N, K = 64, GROUP
    base = torch.full((N, K), -8, dtype=torch.int8)
    assert int(ref.w4_pack(base).abs().sum()) == 0
    seen = set()
    for n in (0, 1, 15, 16, 63):
        for k in range(K):
            q = base.clone()
            q[n, k] = 7
            p = ref.w4_pack(q).to(torch.int64) & 0xFFFFFFFF
            nz = p.nonzero().flatten().tolist()
            assert len(nz) == 1
            word = int(p[nz[0]])
            shift = (word & -word).bit_length() - 1
            assert word == 15 << shift and shift % 4 == 0
            seen.add((nz[0], shift))
    assert len(seen) == 5 * K


def test_pack_rejects_bad_input():
    with pytest.raises(ValueError):
        ref.w4_pack(torch.zeros(64, 64, dtype=torch.int8))      # K % 128
    with pytest.raises(ValueError):
        ref.w4_pack(torch.zeros(32, 128, dtype=torch.int8))     # N % 64
    with pytest.raises(ValueError):
        ref.w4_pack(torch.full((64, 128), 8, dtype=torch.int8))
    with pytest.raises(ValueError):
        ref.w4_unpack(torch.zeros(100, dtype=torch.int32), 64, 128)


def test_quantize_w4_invariants():
    g = torch.Generator().manual_seed(3)
    w = (0.02 * torch.randn(128, 512, generator=g)).to(BF16)
    w[5, 128:256] = 0                       # an all-zero group
    w[7, 0:128] = 0
    w[7, 3] = -0.5                          # one element carries the group
    q, s = ref.quantize_w4(w)
    assert q.dtype == torch.int8 and tuple(q.shape) == (128, 512)
    assert s.dtype == BF16 and tuple(s.shape) == (128, 4)
    assert int(q.min()) >= -8 and int(q.max()) <= 7
    assert bool(torch.isfinite(s.float()).all()) and bool((s.float() > 0).all())
    # the zero group: q = 0 and the smallest positive normal bf16 as scale
    assert int(q[5, 128:256].abs().max()) == 0
    assert float(s[5, 1]) == float(torch.finfo(BF16).tiny)
    # every group's largest element maps to +-7 (bf16(max / 7) is within
    # 2^-8 of max / 7, so max / s is within 7 * 2^-8 of 7)
    wg = w.float().reshape(128, 4, GROUP)
    qg = q.reshape(128, 4, GROUP)
    at = wg.abs().argmax(dim=-1, keepdim=True)
    top = qg.gather(-1, at).squeeze(-1)
    nonzero = wg.abs().amax(dim=-1) > 0
    assert bool((top.abs()[nonzero] == 7).all())
    assert bool((torch.sign(top.float())
                 == torch.sign(wg.gather(-1, at).squeeze(-1)))[nonzero].all())
    assert int(q[7, 3]) == -7
    # round-half-even to the nearest step, inside the clamp
    expect = torch.round(wg / s.float().unsqueeze(-1)).clamp(-8, 7)
    assert torch.equal(qg.float(), expect)
    # reconstruction error at most half a step
    err = (qg.float() * s.float().unsqueeze(-1) - wg).abs()
    assert bool((err <= 0.5 * s.float().unsqueeze(-1) * (1 + 2 ** -7)).all())


def test_quantize_w4_rounds_half_to_even():
    w = torch.zeros(64, 128)
    w[:, 0] = 7.0                           # scale 1
    w[:, 1] = 2.5
    w[:, 2] = 3.5
    w[:, 3] = -0.5
    q, s = ref.quantize_w4(w.to(BF16))
    assert float(s[0, 0]) == 1.0
    assert q[0, :4].tolist() == [7, 2, 4, 0]


@pytest.mark.parametrize("shape", [(1, 64, 128), (17, 192, 1024),
                                   (5, 128, 384)])
def test_w4a16_linear_ref_matches_float64_oracle(shape):
    case = random_case(*shape)
    got = ref.w4a16_linear(case.x, case.packed, case.s)
    assert got.dtype == BF16 and tuple(got.shape) == (shape[0], shape[1])
    y, allowed, _ = random_bound(case)
    err = (got.double() - y).abs()
    assert bool((err <= allowed).all()), float((err / allowed).max())
    # the dispatcher takes the reference on the CPU
    assert torch.equal(ops.w4a16_linear(case.x, case.packed, case.s), got)


def test_w4a16_linear_ref_exact_and_needle_cases():
    """The exact constructions hold on the reference too (they are what
    the device kernel is held to bit for bit)."""
    case = exact_case(17, 192, 1024)
    assert torch.equal(ref.w4a16_linear(case.x, case.packed, case.s),
                       case.expected)
    weights = needle_weights(64, 256)
    case = needle_case(3, 64, 256, weights)
    assert torch.equal(ref.w4a16_linear(case.x, case.packed, case.s),
                       case.expected)


def test_w4a16_linear_ref_scale_multiplies_the_group_partial():
    """Not the dequantized weight: s * q rounded to bf16 first would give
    another result where s * q needs more than 8 significant bits."""
    N, K = 64, 128
    q = torch.full((N, K), 7, dtype=torch.int8)
    s = torch.full((N, 1), 1.0 + 2.0 ** -7, dtype=BF16)     # 8 bits set
    x = torch.zeros(1, K, dtype=BF16)
    x[0, 0] = 1.0
    packed = ref.w4_pack(q)
    got = ref.w4a16_linear(x, packed, s)
    assert float(got[0, 0]) == float(torch.tensor(
        7 * (1.0 + 2.0 ** -7)).to(BF16))
    assert torch.equal(got.double(),
                       oracle64(x, q, s).float().to(BF16).double())


@pytest.mark.parametrize("shape", [(64, 128), (192, 384)])
def test_w4_dequant_ref(shape):
    packed, s, expected = dequant_case(*shape)
    got = ref.w4_dequant(packed, s)
    assert got.dtype == BF16 and torch.equal(got, expected)
    out = torch.empty(shape, dtype=BF16)
    assert ops.w4_dequant(packed, s, out=out) is out
    assert torch.equal(out, expected)
