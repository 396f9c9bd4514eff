"""Input constructions, the float64 oracle and the launcher's documented
K-slicing for the int4-weight (W4A16) tests (a plain helper module,
imported the way tests/gemm_exact_cases.py is).

The oracle is the op's semantic contract in float64:
``y[m, n] = sum_g s[n, g] * sum_{k in g} x[m, k] * q[n, k]``.

* EXACT.  x is ternary in {-1, 0, 1} with at most ``NNZ_MAX`` non-zeros
  per row at random positions, q is uniform in [-8, 7] and every scale is
  a power of two 2^a, a in [-6, 6], per (n, group).  Then every product,
  every group partial and every running total is a multiple of 2^-6 below
  2^18 — an exact f32 value in ANY accumulation order — and that also
  holds for a kernel that carries the weight as 128 + u = 136 + q and
  subtracts 136 * sum(x): its integer group partials stay below
  143 * sum|x| < 2^24.  Both conditions are asserted here on the oracle
  side.  The single RNE rounding to bf16 is then the only rounding, so the
  comparator is ``torch.equal``.
* NEEDLE.  Row m of x is +-1 at one position k_m, q[n, k] takes all 16
  values and every (n, group) has its own scale (consecutive bf16 bit
  patterns), so ``out[m, n] == bf16(+-s[n, g(k_m)] * q[n, k_m])`` bit for
  bit: s * q is exact in f32 (8 + 4 significant bits) and rounds once.  A
  slip in the nibble order, the group index or the scale index shows.
  The positions start with the edges 0, 7, 8, 31, 32, 127, 128, K-1 and
  b-1, b for every K-slice boundary b.
* RANDOM.  x ~ N(0, 1), W ~ 0.02 * N(0, 1) through ``quantize_w4``; the
  bound is ``|got - y64| <= 2^-8 * |y64| + 2^-19 * S`` with
  ``S = sum_g s * sum_k |x| * |q|`` (one bf16 rounding with 2x margin,
  plus f32 accumulation in the offset-binary form).

``plan_slices`` states where the launcher cuts K; it is written from the
kernel's documented contract and imports nothing from the extension.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from resilient_llm_amd.ops import ref

BF16 = torch.bfloat16
SEED = 4321
GROUP = 128
PANEL = 64
NNZ_MAX = 200               # non-zeros per x row of an EXACT case
EDGES = (0, 7, 8, 31, 32, 127, 128)

# (M, N, K): one group; an odd group count; M on both sides of each 16-row
# tile edge; the down-proj K; a wide N
SHAPES = [(1, 64, 128), (3, 64, 256), (16, 128, 384), (17, 192, 1024),
          (33, 64, 2048), (64, 256, 512), (64, 64, 14336), (5, 6144, 256)]
# (M, N, K, splitk): the M <= 16 kernel (weight ring of 4 groups) with more
# than one steady round of its ring and with a tail after it - 7 groups per
# slice (one round + 3), 11 (two rounds + 3, after rounding 32 / 3 up) and
# 8 (two rounds, no tail); the Llama-3-8B down and gate_up projections run
# 7 and 11
RING_SHAPES = [(1, 64, 14336, 16), (16, 64, 4096, 3), (5, 128, 2048, 2)]
RANDOM_SHAPES = [(1, 64, 128), (64, 256, 1024), (16, 64, 4096),
                 (64, 64, 14336)]
DEQUANT_SHAPES = [(64, 128), (192, 384), (6144, 256)]


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# ------------------------------------------------- the launcher's contract
def forced_slices(K: int, splitk: int) -> list:
    """K ranges of the slices when the caller passes ``splitk`` > 0: at most
    one slice per group, ceil(groups / splitk) groups per slice, no empty
    slice."""
    groups = K // GROUP
    per = -(-groups // min(splitk, groups)) * GROUP
    return [(k0, min(k0 + per, K)) for k0 in range(0, K, per)]


def plan_slices(N: int, K: int) -> list:
    """K ranges [(k0, k1), ...] of the slices ``w4a16_linear`` runs: K is
    cut in whole 128-k groups; the launcher wants ceil(1024 / panels)
    slices (panels = N / 64) but keeps at least 4 groups in a slice, a
    slice is ceil(groups / slices) groups, and no slice is empty.  A
    function of (N, K) only."""
    assert N % PANEL == 0 and K % GROUP == 0
    groups, panels = K // GROUP, N // PANEL
    sk = min(max(1, -(-1024 // panels)), max(1, groups // 4))
    per = -(-groups // sk) * GROUP
    return [(k0, min(k0 + per, K)) for k0 in range(0, K, per)]


# ------------------------------------------------------------------ oracle
def oracle64(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor):
    """float64 [M, N] of the contract."""
    M, K = x.shape
    N, G = s.shape
    part = torch.einsum("mgk,ngk->mng", x.double().reshape(M, G, GROUP),
                        q.double().reshape(N, G, GROUP))
    return (part * s.double().unsqueeze(0)).sum(dim=-1)


def abs_sum(x: torch.Tensor, q: torch.Tensor, s: torch.Tensor):
    """S[m, n] = sum_g s * sum_k |x| * |q| (float64)."""
    return oracle64(x.abs(), q.abs(), s)


class Case(NamedTuple):
    name: str
    x: torch.Tensor           # [M, K] bf16
    q: torch.Tensor           # [N, K] int8 in -8..7
    s: torch.Tensor           # [N, K/128] bf16
    packed: torch.Tensor      # int32 [N*K/8]
    expected: torch.Tensor    # [M, N] bf16
    slices: list


def exact_case(M, N, K, seed=SEED, slices=None) -> Case:
    g = _gen(seed + M + 3 * N + 7 * K)
    G = K // GROUP
    nnz = min(K // 2, NNZ_MAX)
    x = torch.zeros(M, K)
    for m in range(M):
        idx = torch.randperm(K, generator=g)[:nnz]
        x[m, idx] = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).float()
    q = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    a = torch.randint(-6, 7, (N, G), generator=g)
    s = torch.exp2(a.float()).to(BF16)
    assert torch.equal(s.float(), torch.exp2(a.float()))
    row_abs = int(x.abs().sum(dim=1).max())
    # the 128 + u representation: integer group partials and totals < 2^24
    assert 143 * row_abs < 2 ** 24, row_abs
    # multiples of 2^-6 (smallest scale) up to 2^6 * 8 * sum|x| < 2^18
    assert 64 * 8 * row_abs < 2 ** 18, row_abs
    x = x.to(BF16)
    y = oracle64(x, q, s)
    expected = y.float().to(BF16)
    assert torch.equal(y.float().double(), y)      # exact in f32
    return Case(f"exact M={M} N={N} K={K}", x, q, s, ref.w4_pack(q),
                expected, slices or plan_slices(N, K))


def needle_positions(K: int, slices, seed=SEED) -> list:
    """Every k in 0..K-1 once: the edges first, then a seeded shuffle."""
    first = list(EDGES) + [K - 1]
    for k0, k1 in slices:
        first += [k0 - 1, k0, k1 - 1, k1]
    head = []
    for k in first:
        if 0 <= k < K and k not in head:
            head.append(k)
    taken = set(head)
    rest = [k for k in torch.randperm(K, generator=_gen(seed)).tolist()
            if k not in taken]
    return head + rest


def n_edge_sweeps(M: int, K: int, slices) -> int:
    """Launches after which every edge position has been a needle."""
    pos = needle_positions(K, slices)
    edges = set(list(EDGES) + [K - 1])
    for k0, k1 in slices:
        edges |= {k0 - 1, k0, k1 - 1, k1}
    n = 1 + max(i for i, k in enumerate(pos) if k in edges)
    return -(-n // M)


def needle_weights(N, K, seed=SEED):
    """(q, s, packed) shared by every sweep of one (N, K): q takes all 16
    values along both n and k, scales are distinct per (n, group)."""
    g = _gen(seed + 11 * N + K)
    G = K // GROUP
    q = ((torch.arange(N)[:, None] * 5 + torch.arange(K)[None, :] * 3
          + torch.randint(0, 16, (1, K), generator=g)) % 16 - 8).to(torch.int8)
    assert len(q.unique()) == 16
    # consecutive bf16 bit patterns from 0x3800 (2^-15) up: N*G <= 12288
    # distinct positive normal values below 2^82
    assert N * G <= 0x3000
    bits = (0x3800 + torch.randperm(N * G, generator=g)).to(torch.int16)
    s = bits.view(BF16).reshape(N, G).contiguous()
    assert len(s.float().unique()) == N * G and bool(s.float().gt(0).all())
    return q, s, ref.w4_pack(q)


def needle_case(M, N, K, weights, sweep=0, seed=SEED, slices=None) -> Case:
    q, s, packed = weights
    slices = slices or plan_slices(N, K)
    g = _gen(seed + 1 + sweep)
    pos = needle_positions(K, slices, seed)
    k_m = torch.tensor([pos[(sweep * M + m) % K] for m in range(M)])
    sign = torch.randint(0, 2, (M,), generator=g) * 2 - 1
    x = torch.zeros(M, K)
    x[torch.arange(M), k_m] = sign.float()
    x = x.to(BF16)
    # closed form: one product per output, exact in f32, rounded once
    closed = (s[:, k_m // GROUP].float() * q[:, k_m].float()).T \
        * sign[:, None].float()
    expected = closed.to(BF16)
    assert torch.equal(oracle64(x, q, s).float().to(BF16), expected)
    return Case(f"needle M={M} N={N} K={K} sweep={sweep} k_m="
                f"{k_m.tolist()[:12]}", x, q, s, packed, expected, slices)


def random_case(M, N, K, seed=SEED) -> Case:
    g = _gen(seed + 2 + M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    w = (0.02 * torch.randn(N, K, generator=g)).to(BF16)
    q, s = ref.quantize_w4(w)
    y = oracle64(x, q, s)
    return Case(f"random M={M} N={N} K={K}", x, q, s, ref.w4_pack(q),
                y.float().to(BF16), plan_slices(N, K))


def random_bound(case: Case):
    """(y64, allowed |got - y64|) of a RANDOM case, both float64 [M, N]."""
    y = oracle64(case.x, case.q, case.s)
    S = abs_sum(case.x, case.q, case.s)
    return y, 2.0 ** -8 * y.abs() + 2.0 ** -19 * S, S


def dequant_case(N, K, seed=SEED):
    """Random q and random bf16 scales (normal, any sign-free exponent in
    2^-20 .. 2^20) -> (packed, s, expected bf16 [N, K])."""
    g = _gen(seed + 5 + N + K)
    G = K // GROUP
    q = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    s = (torch.exp2(torch.randint(-20, 21, (N, G), generator=g).float())
         * (1 + torch.rand(N, G, generator=g))).to(BF16)
    expected = (s.float().repeat_interleave(GROUP, dim=1)
                * q.float()).to(BF16)
    return ref.w4_pack(q), s, expected


def describe(got: torch.Tensor, case: Case) -> str:
    want = case.expected
    bad = got != want
    r, c = bad.nonzero(as_tuple=True)
    first = [(int(i), int(j), float(got[i, j]), float(want[i, j]))
             for i, j in zip(r[:6].tolist(), c[:6].tolist())]
    return (f"{case.name}, slices {case.slices}: {int(bad.sum())} of "
            f"{bad.numel()} wrong ({int(got.isnan().sum())} NaN); rows "
            f"{sorted(set(r.tolist()))[:16]}; 16-col tiles "
            f"{sorted({j // 16 for j in c.tolist()})[:16]}; first (row, col, "
            f"got, expected): {first}")
