"""The zero-point int4 HIP kernels on the device: exact-integer and needle
bit equality (planned and forced K-slicing), poisoned surroundings and
slab, row independence across M, the random-data bound against the
float64 oracle, ``w4_zp_dequant`` and ``awq_repack`` bit equality."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.ops import ref

from awq_cases import (awq_pack, exact_case, layer_case, needle_case,
                       needle_weights, random_bound, random_case)
from w4a16_cases import (BF16, describe, forced_slices, n_edge_sweeps,
                         plan_slices)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 1031            # odd: out starts on no 4-, 8- or 16-byte boundary
# (M, N, K, splitk): one group; an odd group count; every M-tile variant
# and both sides of a 16-row edge; more than one panel; then forced
# slicing with 7 and 11 groups in one slice (ring round + tail, two rounds
# + tail at depth 4) and 8 groups per slice
SHAPES = [(1, 64, 128, 0), (16, 128, 384, 0), (17, 64, 1024, 0),
          (48, 64, 512, 0), (64, 128, 2048, 0), (3, 64, 896, 1),
          (1, 64, 1408, 1), (5, 64, 2048, 2)]
RANDOM_SHAPES = [(1, 64, 128), (64, 128, 1024), (16, 64, 4096)]
ids = lambda s: "x".join(map(str, s))        # noqa: E731


def bits(t):
    return t.contiguous().view(torch.int16)


def slices_of(N, K, splitk):
    sl = forced_slices(K, splitk) if splitk else plan_slices(N, K)
    sk, per = ops.w4a16_plan(N, K, splitk)
    assert (sk, per) == (len(sl), sl[0][1] - sl[0][0])
    return sl


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_integers_bit_equal_and_poison_intact(shape):
    M, N, K, splitk = shape
    case = exact_case(M, N, K, slices=slices_of(N, K, splitk))
    n_ws = len(case.slices) * M * N if len(case.slices) > 1 else 0
    buf = torch.full((2 * GUARD + M * N,), float("nan"), dtype=BF16,
                     device=DEV)
    wbuf = torch.full((2 * (GUARD + 1) + n_ws,), float("nan"),
                      dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + M * N].view(M, N)
    ws = wbuf[GUARD + 1:GUARD + 1 + n_ws] if n_ws else None
    x, packed, meta = (t.to(DEV) for t in (case.x, case.packed, case.meta))
    got = ops.w4a16_zp_linear(x, packed, meta, splitk, out=out, ws=ws)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), case.expected), describe(out.cpu(), case)
    host, whost = buf.cpu().isnan(), wbuf.cpu().isnan()
    assert bool(host[:GUARD].all() and host[GUARD + M * N:].all())
    assert bool(whost[:GUARD + 1].all() and whost[GUARD + 1 + n_ws:].all())
    assert not bool(whost[GUARD + 1:GUARD + 1 + n_ws].any())
    # the op's own allocations give the same bits
    assert torch.equal(bits(ops.w4a16_zp_linear(x, packed, meta, splitk)),
                       bits(out))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_needles_bit_equal(shape):
    """out[m, n] == bf16(+-s[n, g] * (u[n, k_m] - z[n, g])) for needles at
    0, 7, 8, 31, 32, 127, 128, K-1 and both sides of every slice edge."""
    M, N, K, splitk = shape
    slices = slices_of(N, K, splitk)
    weights = needle_weights(N, K)
    first = needle_case(M, N, K, weights, 0, slices=slices)
    packed, meta = first.packed.to(DEV), first.meta.to(DEV)
    for sweep in range(n_edge_sweeps(M, K, slices)):
        case = needle_case(M, N, K, weights, sweep, slices=slices)
        out = ops.w4a16_zp_linear(case.x.to(DEV), packed, meta, splitk).cpu()
        assert torch.equal(out, case.expected), describe(out, case)


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=ids)
def test_random_bf16_within_the_bound(shape):
    """|got - y64| <= 2^-8 |y64| + 2^-19 S, S = sum s sum |x| |u - z|."""
    case = random_case(*shape)
    got = ops.w4a16_zp_linear(case.x.to(DEV), case.packed.to(DEV),
                              case.meta.to(DEV)).cpu().double()
    y, allowed, S = random_bound(case)
    err = (got - y).abs()
    half_ulp = torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(1e-300)))
                          - 8)
    acc = ((err - half_ulp).clamp_min(0) / S).max()
    print(f"w4a16_zp random {shape}: max err/allowed "
          f"{float((err / allowed).max()):.3f}, max (err - half ulp)/S "
          f"{float(acc):.3e}")
    assert bool((err <= allowed).all()), float((err / allowed).max())


def test_row_m_of_64_is_the_single_row_launch():
    case = random_case(64, 128, 1024)
    x, packed, meta = (t.to(DEV) for t in (case.x, case.packed, case.meta))
    full = ops.w4a16_zp_linear(x, packed, meta)
    for m in (0, 15, 16, 63):
        one = ops.w4a16_zp_linear(x[m:m + 1].contiguous(), packed, meta)
        assert torch.equal(bits(full[m:m + 1]), bits(one)), m


@pytest.mark.parametrize("shape", [(64, 128), (192, 384)], ids=ids)
def test_dequant_and_repack_bit_equal(shape):
    N, K = shape
    u, z, s, w = layer_case(N, K)
    packed, meta = ref.w4_pack(u.to(torch.int8) - 8), ref.w4_zp_meta(z, s)
    buf = torch.full((2 * GUARD + N * K,), float("nan"), dtype=BF16,
                     device=DEV)
    out = buf[GUARD:GUARD + N * K].view(N, K)
    ops.w4_zp_dequant(packed.to(DEV), meta.to(DEV), out=out)
    torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.equal(bits(host[GUARD:GUARD + N * K].view(N, K)), bits(w))
    assert bool(host[:GUARD].isnan().all() and host[GUARD + N * K:].isnan().all())
    # the device repack of the AutoAWQ tensors gives the same pair
    qw, qz, sc = awq_pack(u, z, s)
    uu, zz, ss = ref.awq_unpack(qw, qz, sc)
    p_d = torch.zeros(N * K // 8, dtype=torch.int32, device=DEV)
    m_d = torch.zeros((N, K // 128), dtype=torch.int32, device=DEV)
    ops.awq_repack(qw.to(DEV), qz.to(DEV), sc.to(DEV), p_d, m_d, 0)
    assert torch.equal(p_d.cpu(), ref.w4_pack(uu.to(torch.int8) - 8))
    assert torch.equal(m_d.cpu(), ref.w4_zp_meta(zz, ss))
    assert torch.equal(p_d.cpu(), packed) and torch.equal(m_d.cpu(), meta)


def test_repack_writes_fused_slices_at_their_offsets():
    """Three column slices (128 / 64 / 64, as q / k / v) into one N = 256
    output: after every write the columns not yet written keep their
    poison."""
    K, G, POISON = 384, 3, 0x5A5A5A5A
    p_d = torch.full((256 * K // 8,), POISON, dtype=torch.int32, device=DEV)
    m_d = torch.full((256, G), POISON, dtype=torch.int32, device=DEV)
    want_p, want_m = p_d.cpu().clone(), m_d.cpu().clone()
    for width, col, seed in ((64, 128, 1), (128, 0, 2), (64, 192, 3)):
        u, z, s, _ = layer_case(width, K, seed=seed)
        qw, qz, sc = awq_pack(u, z, s)
        ops.awq_repack(qw.to(DEV), qz.to(DEV), sc.to(DEV), p_d, m_d, col)
        uu, zz, ss = ref.awq_unpack(qw, qz, sc)
        want_p[col * K // 8:(col + width) * K // 8] = ref.w4_pack(
            uu.to(torch.int8) - 8)
        want_m[col:col + width] = ref.w4_zp_meta(zz, ss)
        assert torch.equal(p_d.cpu(), want_p), col
        assert torch.equal(m_d.cpu(), want_m), col
    assert not bool((want_m == POISON).any())
    with pytest.raises(RuntimeError, match="col_offset"):
        ops.awq_repack(qw.to(DEV), qz.to(DEV), sc.to(DEV), p_d, m_d, 224)
