"""Exact-integer input constructions, the float64 oracle and the
bit-exact comparator for tests/test_gemm_exact.py (a plain helper
module, imported the way tests/attn_boundary_cases.py is).

Every construction makes the GEMM result EXACT: all products and all
partial sums are integers far below 2^24 times ONE power of two per
output element, so any f32 accumulation order - split-K or not, MFMA or
scalar - gives the same f32 value, and the single RNE rounding to bf16
leaves it unchanged.  The oracle is
``(x.double() @ w.double().T).float().bfloat16()`` and the comparator
is ``torch.equal``: no tolerance anywhere.

* TERNARY (a k dropped or counted twice).  x and W are i.i.d. uniform
  in {-1, 0, 1}.  The oracle must stay within |y| <= 256 (asserted), so
  every value is a bf16-exact integer and an error of 1 is visible.  For
  K > 3584 each x element is kept with probability 1/4 to stay there.
* NEEDLE (index mapping, mantissa pass-through).  Row m of x is +-1 at
  one position k_m, W holds odd integers in [-255, 255] (all 8 mantissa
  bits), so out[m, n] == +-W[n, k_m] bit for bit.  The positions start
  with the edges 0, 7, 8, 31, 32, 255, 256, K-1 and b-1, b for every
  K-slice boundary b of the case; a seeded permutation of the remaining
  k follows, and ``sweep`` moves on by M positions per launch, so
  ceil(K / M) launches make every k a needle.
* SCALED (exponent handling).  TERNARY with row m of x times 2^a_m and
  row n of W times 2^b_n, a and b in [-6, 6]: the TERNARY result times
  2^(a_m + b_n), still exact.
* SILU coding, for the fused silu(gate) * up prologue: an activation t
  becomes gu = [gate | up] with gate = 32, up = t/32 where t != 0
  (silu(32) == 32 exactly in f32: 1 + exp(-32) == 1), and by coin flip
  gate = 0, up = +-1/32 or gate = 32, up = 0 where t == 0.  No negative
  gates: silu(-32) * u is a tiny non-zero that would break exactness.

``split_slices`` states where the launchers cut K, and ``v1_splitk`` /
``v2_splitk`` how many f32 slabs the ops allocate; both are written from
the kernels' documented contract and import nothing from the extension.
``python -m tests.gemm_exact_cases --v2-sweep`` is the child process of
the granule-ring test (RLLI_SK2_G is read once per process).
"""

from __future__ import annotations

import sys
from typing import NamedTuple

import torch

BF16 = torch.bfloat16
SEED = 1234
CAP = 256                   # largest |y| of a TERNARY oracle
PANEL = 64                  # output columns per workgroup / wave
TILE = 16                   # MFMA tile: rows and columns
GRANULE = 32                # k per MFMA
DENSE_K_MAX = 3584          # dense ternary x up to here, 1/4 density above
EDGES = (0, 7, 8, 31, 32, 255, 256)


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# ------------------------------------------------- the launchers' contract
def split_slices(K: int, splitk: int, unit: int = 256) -> list:
    """K ranges [(k0, k1), ...] of the slices a launcher runs: K is cut in
    chunks of ``unit``, a slice is ceil(chunks / splitk) chunks, and a
    slice that would start at or past K does not exist (its slab must not
    be summed).  len(result) <= splitk."""
    assert splitk >= 1 and K % unit == 0 and K >= unit, (K, splitk, unit)
    per = -(-(K // unit) // splitk) * unit
    return [(k0, min(k0 + per, K)) for k0 in range(0, K, per)]


def v1_splitk(N: int, K: int) -> int:
    """Slab count ``skinny_linear`` allocates: fill ~512 workgroups of 64
    columns, at most 8 slices, at most one per 256 k; none from 256
    panels up."""
    panels = N // PANEL
    if panels >= 256:
        return 1
    return min(8, max(1, 512 // panels), K // 256)


def v2_splitk(N: int, K: int, splitk: int = 0) -> int:
    """Slab count ``skinny2_linear`` / ``skinny2_silu_linear`` allocate:
    the caller's splitk, or ceil(512 / panels) when it is <= 0, clamped
    to one slice per 256 k."""
    panels = N // PANEL
    sk = splitk if splitk > 0 else max(1, -(-512 // panels))
    return max(1, min(sk, K // 256))


# ------------------------------------------------------------ constructions
class Case(NamedTuple):
    name: str
    x: torch.Tensor           # [M, K] bf16 activation (before SILU coding)
    w: torch.Tensor           # [N, K] bf16
    expected: torch.Tensor    # [M, N] bf16
    slices: list              # K ranges of the launch (for the report)


def oracle(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return (x.double() @ w.double().T).float().bfloat16()


def _ternary(shape, g, density: float = 1.0) -> torch.Tensor:
    t = torch.randint(-1, 2, shape, generator=g, dtype=torch.int8)
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density)
    return t.to(BF16)


def _ternary_xw(M, N, K, seed):
    g = _gen(seed)
    x = _ternary((M, K), g, 1.0 if K <= DENSE_K_MAX else 0.25)
    w = _ternary((N, K), g)
    y = oracle(x, w)
    peak = float(y.abs().max())
    assert peak <= CAP, (
        f"TERNARY M={M} N={N} K={K} seed={seed}: max|y| = {peak} > {CAP}; "
        f"change the density or the seed, not the cap")
    return x, w, y


def ternary_case(M, N, K, slices=None, seed=SEED) -> Case:
    x, w, y = _ternary_xw(M, N, K, seed)
    return Case(f"ternary M={M} N={N} K={K}", x, w, y,
                slices or [(0, K)])


def needle_positions(K: int, slices=None, seed=SEED) -> list:
    """Every k in 0..K-1 once: the edges first, then a seeded shuffle."""
    first = list(EDGES) + [K - 1]
    for k0, k1 in (slices or []):
        first += [k0 - 1, k0, k1 - 1, k1]
    head = []
    for k in first:
        if 0 <= k < K and k not in head:
            head.append(k)
    taken = set(head)
    rest = [k for k in torch.randperm(K, generator=_gen(seed)).tolist()
            if k not in taken]
    return head + rest


def needle_case(M, N, K, slices=None, sweep=0, seed=SEED) -> Case:
    g = _gen(seed + 1)
    pos = needle_positions(K, slices, seed)
    k_m = torch.tensor([pos[(sweep * M + m) % K] for m in range(M)])
    sign = torch.randint(0, 2, (M,), generator=g) * 2 - 1
    x = torch.zeros(M, K)
    x[torch.arange(M), k_m] = sign.float()
    w = (torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int16)
         * 2 + 1).to(BF16)
    x = x.to(BF16)
    y = oracle(x, w)
    closed = (w[:, k_m].T.float() * sign[:, None]).to(BF16)
    assert torch.equal(y, closed)
    return Case(f"needle M={M} N={N} K={K} sweep={sweep} k_m="
                f"{k_m.tolist()[:12]}", x, w, y, slices or [(0, K)])


def n_edge_sweeps(M: int, K: int, slices=None) -> int:
    """Launches after which every edge position has been a needle."""
    pos = needle_positions(K, slices)
    edges = set(list(EDGES) + [K - 1])
    for k0, k1 in (slices or []):
        edges |= {k0 - 1, k0, k1 - 1, k1}
    n = 1 + max(i for i, k in enumerate(pos) if k in edges)
    return -(-n // M)


def scaled_case(M, N, K, slices=None, seed=SEED) -> Case:
    x, w, y = _ternary_xw(M, N, K, seed)
    g = _gen(seed + 2)
    a = torch.randint(-6, 7, (M,), generator=g)
    b = torch.randint(-6, 7, (N,), generator=g)
    xs = (x.float() * torch.exp2(a.float())[:, None]).to(BF16)
    ws = (w.float() * torch.exp2(b.float())[:, None]).to(BF16)
    ys = oracle(xs, ws)
    scale = torch.exp2((a[:, None] + b[None, :]).float())
    assert torch.equal(ys.float(), y.float() * scale)
    return Case(f"scaled M={M} N={N} K={K}", xs, ws, ys, slices or [(0, K)])


def encode_silu(t: torch.Tensor, seed=SEED) -> torch.Tensor:
    """gu = [gate | up] bf16 with silu(gate) * up == t exactly."""
    g = _gen(seed + 3)
    tf = t.float()
    nz = tf != 0
    coin = torch.rand(t.shape, generator=g) < 0.5
    sign = (torch.randint(0, 2, t.shape, generator=g) * 2 - 1).float()
    gate = torch.where(nz | ~coin, 32.0, 0.0)
    up = torch.where(nz, tf / 32, torch.where(coin, sign / 32, 0.0))
    gu = torch.cat([gate, up], dim=-1).to(BF16)
    assert torch.equal(gu.float(), torch.cat([gate, up], dim=-1))
    return gu


def case_input(case: Case, kind: str) -> torch.Tensor:
    """What a backend of this kind ("plain" / "silu") is given as x."""
    return encode_silu(case.x) if kind == "silu" else case.x


# --------------------------------------------------------------- comparator
def _compact(idx) -> str:
    idx = sorted(set(int(i) for i in idx))
    runs, start, prev = [], None, None
    for i in idx:
        if start is None:
            start = prev = i
        elif i == prev + 1:
            prev = i
        else:
            runs.append((start, prev))
            start = prev = i
    if start is not None:
        runs.append((start, prev))
    txt = ", ".join(str(a) if a == b else f"{a}-{b}" for a, b in runs[:16])
    return txt + (", ..." if len(runs) > 16 else "")


class Mismatch(NamedTuple):
    count: int
    numel: int
    nan: int
    rows: list
    cols: list
    panels: list              # 64-column panels
    tiles: list               # 16-column tiles
    first: list               # (row, col, got, expected)
    hints: list               # K ranges the difference is consistent with

    def __str__(self):
        s = (f"{self.count} of {self.numel} elements wrong ({self.nan} NaN); "
             f"rows {_compact(self.rows)}; cols {_compact(self.cols)}; "
             f"64-col panels {_compact(self.panels)}; "
             f"16-col tiles {_compact(self.tiles)}; "
             f"first (row, col, got, expected): {self.first}")
        if self.hints:
            s += "; " + "; ".join(self.hints)
        return s


def _k_hints(d, bad, case: Case) -> list:
    """Name the K range whose partial product the difference equals."""
    K = case.x.shape[1]
    named = [(f"slice {i} = k[{k0}, {k1})", k0, k1)
             for i, (k0, k1) in enumerate(case.slices)]
    named.append((f"last granule = k[{K - GRANULE}, {K})", K - GRANULE, K))
    xd, wd = case.x.double(), case.w.double()
    hints = []
    for name, k0, k1 in named:
        part = xd[:, k0:k1] @ wd[:, k0:k1].T
        if not torch.equal(bad, part != 0):
            continue
        if torch.equal(d[bad], -part[bad]):
            hints.append(f"difference == minus the partial sum of {name} "
                         f"(dropped)")
        elif torch.equal(d[bad], part[bad]):
            hints.append(f"difference == the partial sum of {name} "
                         f"(counted twice)")
    return hints


def compare(got: torch.Tensor, case: Case, n_first: int = 6):
    """None when ``got`` is bit-for-bit the oracle (torch.equal), else a
    Mismatch naming where it is not."""
    want = case.expected
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (
        got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    if torch.equal(got, want):
        return None
    bad = got != want                    # NaN != anything: counted
    r, c = bad.nonzero(as_tuple=True)
    rows, cols = r.unique().tolist(), c.unique().tolist()
    first = [(int(i), int(j), float(got[i, j]), float(want[i, j]))
             for i, j in zip(r[:n_first].tolist(), c[:n_first].tolist())]
    nan = int(got.isnan().sum())
    hints = []
    if nan == 0:
        hints = _k_hints(got.double() - want.double(), bad, case)
    return Mismatch(int(bad.sum()), bad.numel(), nan, rows, cols,
                    sorted({j // PANEL for j in cols}),
                    sorted({j // TILE for j in cols}), first, hints)


def assert_exact(got: torch.Tensor, case: Case, what: str) -> None:
    bad = compare(got, case)
    if bad is not None:
        raise AssertionError(f"{what}, {case.name}, slices {case.slices}: "
                             f"{bad}")


# ------------------------------------------- child of the granule-ring test
def _v2_sweep() -> int:
    """TERNARY and NEEDLE through both v2 kernels at whatever ring depth
    RLLI_SK2_G selects for this process; 1 on any mismatch."""
    import os
    import resilient_llm_amd.ops as ops
    fns = {"plain": ops.skinny2_linear, "silu": ops.skinny2_silu_linear}
    N, failed, ran = 128, 0, 0
    for M in (1, 17, 33, 64):
        for K in (256, 768):
            # splitk 1: 8 / 24 granules in one slice, so every ring depth
            # reaches its steady state; 0 (auto): one slice per 256 k
            for sk in (1, 0):
                sl = split_slices(K, v2_splitk(N, K, sk))
                for case in (ternary_case(M, N, K, sl),
                             needle_case(M, N, K, sl)):
                    w = case.w.cuda()
                    for kind, fn in fns.items():
                        out = fn(case_input(case, kind).cuda(), w, sk)
                        bad = compare(out, case)
                        ran += 1
                        if bad is not None:
                            failed += 1
                            print(f"MISMATCH {kind} splitk={sk} {case.name} "
                                  f"slices {sl}: {bad}", flush=True)
    print(f"v2 sweep RLLI_SK2_G={os.environ.get('RLLI_SK2_G')}: "
          f"{ran} runs, {failed} wrong", flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    if sys.argv[1:] != ["--v2-sweep"]:
        sys.exit("usage: python -m tests.gemm_exact_cases --v2-sweep")
    sys.exit(_v2_sweep())
