"""Exact-integer and poisoned-workspace tests of the decode GEMMs
(skinny_gemm.hip, skinny2.hip, lt_gemm.cpp, ops/autotune.py).

Random inputs with a bf16 tolerance cannot see a dropped 32-k granule, a
row guard off by one or a stale split-K slab.  These tests use inputs
whose result is exact in bf16 (tests/gemm_exact_cases.py: TERNARY,
NEEDLE, SCALED and the SILU coding) and compare with ``torch.equal``.
The first half runs on the CPU and gives the GPU half its meaning: the
comparator accepts the project's CPU fallbacks and REJECTS deliberately
wrong results, naming where they are wrong.  No deliberately broken
kernel is ever run on a GPU.

A new GEMM kernel joins every sweep by adding one ``Backend`` row to
BACKENDS below (callable, "plain" / "silu" input coding, its split-K
family); nothing else in this file has to change.
"""

import os
import subprocess
import sys
from typing import Callable, NamedTuple, Optional

import pytest
import torch

import resilient_llm_amd.ops as ops
from resilient_llm_amd.ops import autotune, ref
from tests import gemm_exact_cases as C

DEV = "cuda"
REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDLE_MS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)


# ============================================================ backend table
class Backend(NamedTuple):
    name: str
    call: Callable            # (x or gu, w, splitk) -> out [M, N] bf16
    kind: str                 # input coding: "plain" (x) or "silu" ([g|u])
    takes_splitk: bool
    family: Optional[str]     # split-K sweep it belongs to: "v1", "v2"
    cpu: bool                 # has a CPU fallback
    max_m: int = 64           # constraints: M <= max_m,
    k_mult: int = 256         # K % k_mult == 0,
    n_mult: int = 64          # N % n_mult == 0


def _lt(rank):
    """hipBLASLt with the rank-th algorithm of its own heuristic list."""
    def call(x, w, splitk=0):
        ops.load_extension(required=True)
        idxs = torch.ops.rlli.lt_heuristics(x, w, 4).tolist()
        assert idxs, "no hipblaslt heuristics returned"
        call.algo = idxs[min(rank, len(idxs) - 1)]
        return torch.ops.rlli.lt_linear(x, w, call.algo)
    call.algo = None
    return call


BACKENDS = [
    Backend("skinny_linear", lambda x, w, sk=0: ops.skinny_linear(x, w),
            "plain", False, "v1", True),
    Backend("linear_auto", lambda x, w, sk=0: ops.linear_auto(x, w),
            "plain", False, "v1", False),
    Backend("skinny2_linear", ops.skinny2_linear, "plain", True, "v2", True),
    Backend("skinny2_silu_linear", ops.skinny2_silu_linear, "silu", True,
            "v2", True),
    Backend("lt_linear#0", _lt(0), "plain", False, None, False, 1 << 30, 1, 1),
    Backend("lt_linear#1", _lt(1), "plain", False, None, False, 1 << 30, 1, 1),
    Backend("lt_linear#2", _lt(2), "plain", False, None, False, 1 << 30, 1, 1),
    Backend("tuned_linear", lambda x, w, sk=0: autotune.tuned_linear(x, w),
            "plain", False, None, False, 1 << 30, 1, 1),
]
_ids = [b.name for b in BACKENDS]
CPU_BACKENDS = [b for b in BACKENDS if b.cpu]
V1 = [b for b in BACKENDS if b.family == "v1"]
V2 = [b for b in BACKENDS if b.family == "v2"]


def slices_of(be, N, K, splitk=0, unit=256):
    """K ranges the backend's launcher cuts this problem into."""
    if be.family == "v1":
        return C.split_slices(K, C.v1_splitk(N, K), unit)
    if be.family == "v2":
        return C.split_slices(K, C.v2_splitk(N, K, splitk))
    return [(0, K)]


def what(be, splitk=None):
    s = be.name
    if be.takes_splitk and splitk is not None:
        s += f" splitk={splitk}"
    if getattr(be.call, "algo", None) is not None:
        s += f" (hipBLASLt algo index {be.call.algo})"
    return s


def run(be, case, splitk=0, w_dev=None, dev="cpu"):
    M, K = case.x.shape
    N = case.w.shape[0]
    assert M <= be.max_m and K % be.k_mult == 0 and N % be.n_mult == 0
    w = case.w.to(dev) if w_dev is None else w_dev
    return be.call(C.case_input(case, be.kind).to(dev), w, splitk)


# =========================================================== CPU: contract
def test_split_slices_contract():
    assert C.split_slices(2304, 8) == [
        (0, 512), (512, 1024), (1024, 1536), (1536, 2048), (2048, 2304)]
    assert C.split_slices(1280, 4) == [(0, 512), (512, 1024), (1024, 1280)]
    assert C.split_slices(3584, 8) == [(k, k + 512) for k in range(0, 3584, 512)]
    assert len(C.split_slices(7168, 8)) == 7
    assert len(C.split_slices(2304, 8, unit=128)) == 6
    assert C.split_slices(256, 1) == [(0, 256)]
    for K in range(256, 15 * 256, 256):
        for sk in range(1, 9):
            sl = C.split_slices(K, sk)
            assert len(sl) <= sk and sl[0][0] == 0 and sl[-1][1] == K
            assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
            assert all(k0 < k1 and k0 % 256 == 0 for k0, k1 in sl)
    # the slab counts the issue's v1 sweep relies on
    assert [C.v1_splitk(n, 3584) for n in
            (64, 4096, 6400, 8192, 11008, 16384)] == [8, 8, 5, 4, 2, 1]
    assert C.v1_splitk(64, 512) == 2 and C.v1_splitk(64, 256) == 1
    assert C.v2_splitk(64, 1280, 4) == 4 and C.v2_splitk(64, 512, 8) == 2
    assert C.v2_splitk(4096, 3584, 0) == 8 and C.v2_splitk(192, 3584) == 14


def test_constructions_are_exact():
    sl = C.split_slices(768, 3)
    for case in (C.ternary_case(33, 192, 768, sl),
                 C.needle_case(33, 192, 768, sl),
                 C.scaled_case(33, 192, 768, sl)):
        # bf16 holds every input and the f32 matmul of them is the oracle
        y32 = case.x.float() @ case.w.float().T
        assert torch.equal(y32, case.x.double() @ case.w.double().T)
        assert torch.equal(y32.bfloat16().float(), y32), case.name
        # SILU coding: the reference activation gives x back bit for bit,
        # the swapped halves do not
        gu = C.encode_silu(case.x)
        assert torch.equal(ref.silu_mul(gu), case.x), case.name
        g, u = gu.chunk(2, -1)
        assert not torch.equal(ref.silu_mul(torch.cat([u, g], -1)), case.x)
        assert (g >= 0).all()
    w = C.needle_case(4, 64, 256).w.float()
    assert (w % 2 == 1).all() and w.abs().max() <= 255
    assert len(w.abs().unique()) == 128           # all 8 mantissa bits
    # sparse x keeps K = 7168 (Llama-8B down-proj at TP=2) under the cap
    assert C.ternary_case(64, 1024, 7168).expected.abs().max() <= C.CAP


def test_needle_positions_cover_edges_and_every_k():
    sl = C.split_slices(2304, 8)
    pos = C.needle_positions(2304, sl)
    assert sorted(pos) == list(range(2304))
    assert pos[:8] == [0, 7, 8, 31, 32, 255, 256, 2303]
    for k0, k1 in sl[1:]:
        assert {k0 - 1, k0} <= set(pos[:8 + 4 * len(sl)])
    M, K = 64, 512
    seen = set()
    for s in range(K // M):
        x = C.needle_case(M, 64, K, sweep=s).x
        assert (x != 0).sum(1).tolist() == [1] * M
        seen |= set(x.float().abs().argmax(1).tolist())
    assert seen == set(range(K))
    assert C.n_edge_sweeps(1, 512) == 8 and C.n_edge_sweeps(64, 512) == 1


@pytest.mark.parametrize("be", CPU_BACKENDS, ids=[b.name for b in CPU_BACKENDS])
@pytest.mark.parametrize("make", [C.ternary_case, C.needle_case, C.scaled_case],
                         ids=["ternary", "needle", "scaled"])
def test_comparator_accepts_cpu_fallback(be, make):
    for M, N, K in [(1, 64, 256), (33, 192, 768), (64, 128, 2304)]:
        case = make(M, N, K, slices_of(be, N, K))
        C.assert_exact(run(be, case), case, what(be))


# ---------------------------------------------- deliberately wrong results
M_, N_, K_ = 33, 192, 768
SL_ = C.split_slices(K_, 3)
MAKERS = {"ternary": C.ternary_case, "needle": C.needle_case,
          "scaled": C.scaled_case}


def _y32(case):
    return case.x.float() @ case.w.float().T


def _last_granule_dropped(case):
    return case.x[:, :-32].float() @ case.w[:, :-32].float().T


def _slice_dropped(case):
    k0, k1 = SL_[1]
    return _y32(case) - case.x[:, k0:k1].float() @ case.w[:, k0:k1].float().T


def _slice_twice(case):
    k0, k1 = SL_[2]
    return _y32(case) + case.x[:, k0:k1].float() @ case.w[:, k0:k1].float().T


def _rows_swapped(case):
    y = _y32(case)
    y[[15, 16]] = y[[16, 15]]
    return y


def _tile_shifted(case):
    y = _y32(case)
    y[:, 16:32] = y[:, 16:32].roll(1, dims=1)
    return y


def _slab_small(case):
    y = _y32(case)
    y[:, 64:128] += 1e-3
    return y


def _slab_nan(case):
    y = _y32(case)
    y[16:32, 128:192] += float("nan")
    return y


@pytest.mark.parametrize("kind", ["ternary", "needle", "scaled"])
@pytest.mark.parametrize("fault", [
    "last_granule_dropped", "slice_dropped", "slice_twice", "rows_swapped",
    "tile_shifted", "slab_small", "slab_nan"])
def test_comparator_rejects_wrong_result(fault, kind):
    if fault == "slab_small" and kind == "needle":
        # NEEDLE outputs are odd integers, never 0: y + 1e-3 rounds back to
        # y in bf16.  Seeing a small stale slab is TERNARY's job (about one
        # output in 50 is 0 there), which is why the poison tests use it.
        case = C.needle_case(M_, N_, K_, SL_)
        assert C.compare(_slab_small(case).bfloat16(), case) is None
        return
    case = MAKERS[kind](M_, N_, K_, SL_)
    got = globals()["_" + fault](case).bfloat16()
    bad = C.compare(got, case)
    assert bad is not None, f"{fault} not rejected on {case.name}"
    with pytest.raises(AssertionError, match="elements wrong"):
        C.assert_exact(got, case, fault)
    text = str(bad)
    cols = set(bad.cols)
    zero = (case.expected == 0)
    if fault == "last_granule_dropped":
        assert "last granule = k[736, 768)" in text and "dropped" in text
    elif fault == "slice_dropped":
        assert "slice 1 = k[256, 512)" in text and "(dropped)" in text
        assert "slice 0" not in text and "slice 2" not in text
    elif fault == "slice_twice":
        assert "slice 2 = k[512, 768)" in text and "(counted twice)" in text
        assert "slice 0" not in text and "slice 1" not in text
    elif fault == "rows_swapped":
        assert bad.rows == [15, 16] and "rows 15-16;" in text
    elif fault == "tile_shifted":
        assert bad.tiles == [1] and bad.panels == [0]
        assert cols <= set(range(16, 32)) and len(cols) >= 15
        assert "16-col tiles 1;" in text
    elif fault == "slab_small":
        assert bad.panels == [1] and cols <= set(range(64, 128))
        assert "64-col panels 1;" in text
        # every zero of the slab shows the stale 1e-3
        assert bad.count >= int(zero[:, 64:128].sum()) > 0
        # 1e-3 is above half a bf16 ulp only below 2^-1
        assert all(abs(w) < 0.5 for *_, w in bad.first)
    elif fault == "slab_nan":
        assert bad.nan == bad.count == 16 * 64
        assert bad.rows == list(range(16, 32)) and bad.panels == [2]
        assert "rows 16-31;" in text and "64-col panels 2;" in text
    # a dropped / doubled K range is wrong exactly where its partial is not 0
    if fault in ("slice_dropped", "slice_twice", "last_granule_dropped"):
        assert bad.count == int((got != case.expected).sum()) > 0
        assert bad.first[0][2] != bad.first[0][3]


@pytest.mark.parametrize("kind", ["ternary", "needle", "scaled"])
def test_comparator_rejects_gate_up_swapped(kind):
    case = MAKERS[kind](M_, N_, K_, SL_)
    g, u = C.encode_silu(case.x).chunk(2, -1)
    got = torch.nn.functional.linear(
        ref.silu_mul(torch.cat([u, g], -1)), case.w)
    bad = C.compare(got, case)
    assert bad is not None
    # the swapped activation is silu(t/32) * 32 ~ t/2: wrong wherever the
    # result is not 0, in every row and every panel
    assert bad.count >= int((case.expected != 0).sum()) * 0.9
    assert bad.rows == list(range(M_)) and bad.panels == [0, 1, 2]


# ==================================================================== GPU
@pytest.fixture(autouse=True)
def _tuner_on(monkeypatch):
    """tuned_linear races the hipBLASLt candidates only when opted in;
    the shapes it tunes here stay out of the process-wide cache."""
    monkeypatch.setattr(autotune, "_DISABLED", False)
    monkeypatch.setattr(autotune, "_cache", {})
    monkeypatch.setattr(autotune, "_candidates", {})


def poisoned_run(be, case, splitk, alloc, w_dev):
    """Run with NaN in the blocks the op is about to allocate: its bf16
    output and its ``alloc`` f32 split-K slabs.  The caching allocator
    hands a freed block back to the next request of the same size, which
    the output pointer verifies."""
    M, N = case.expected.shape
    inp = C.case_input(case, be.kind).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    p_out = torch.full((M * N,), float("nan"), dtype=torch.bfloat16,
                       device=DEV)
    p_ws = (torch.full((alloc * M * N,), float("nan"), dtype=torch.float32,
                       device=DEV) if alloc > 1 else None)
    ptr = p_out.data_ptr()
    del p_out, p_ws
    out = be.call(inp, w_dev, splitk)
    assert out.data_ptr() == ptr, (
        f"{what(be, splitk)}, {case.name}: the poison did not land where "
        f"the op allocates its output")
    return out


def _report(failures):
    assert not failures, (f"{len(failures)} wrong; first: "
                          + "\n".join(failures[:6]))


def _collect(failures, out, case, label):
    bad = C.compare(out, case)
    if bad is not None:
        failures.append(f"{label}, {case.name}, slices {case.slices}: {bad}")


@pytest.mark.gpu
@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
def test_m_sweep(be):
    """Every M in 1..64 (all four 16-row tiles and their edges)."""
    N, K = 128, 512
    sl = slices_of(be, N, K)
    failures = []
    for M in range(1, 65):
        cases = [C.ternary_case(M, N, K, sl)]
        if M in NEEDLE_MS:
            # M = 64: every k of K is a needle once; else every edge is
            n = K // M if M == 64 else C.n_edge_sweeps(M, K, sl)
            cases += [C.needle_case(M, N, K, sl, sweep=s) for s in range(n)]
        for case in cases:
            _collect(failures, run(be, case, dev=DEV), case, what(be))
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("be", V2, ids=[b.name for b in V2])
def test_v2_splitk_sweep_poisoned(be, M, N):
    """skinny2.hip: even, uneven, clamped and empty-trailing splits, each
    with NaN in the output and in every slab the op allocates."""
    failures = []
    for chunks in (1, 2, 3, 5, 7, 9, 14):
        K = chunks * 256
        for sk in (0, 1, 2, 3, 4, 5, 8):
            alloc = C.v2_splitk(N, K, sk)
            sl = C.split_slices(K, alloc)
            tern = C.ternary_case(M, N, K, sl)
            w_dev = tern.w.to(DEV)
            out = poisoned_run(be, tern, sk, alloc, w_dev)
            _collect(failures, out, tern, what(be, sk))
            need = C.needle_case(M, N, K, sl)
            _collect(failures, run(be, need, sk, dev=DEV), need, what(be, sk))
    _report(failures)


V1_SWEEP = [(n, None) for n in (64, 4096, 6400, 8192, 11008, 16384)] + [
    (n, env) for env in ("RLLI_SKINNY_KC=128", "RLLI_SKINNY_WDEPTH=1")
    for n in (64, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,env", V1_SWEEP,
                         ids=[f"{n}-{e or 'default'}" for n, e in V1_SWEEP])
def test_v1_splitk_sweep_poisoned(N, env, monkeypatch):
    """skinny_gemm.hip picks splitk from N (8, 8, 5, 4, 2, 1 here); the
    launcher reads both variables on every call."""
    unit = 256
    if env:
        name, val = env.split("=")
        monkeypatch.setenv(name, val)
        unit = 128 if name == "RLLI_SKINNY_KC" else 256
    failures = []
    for chunks in (1, 2, 9, 14):
        K = chunks * 256
        alloc = C.v1_splitk(N, K)
        sl = C.split_slices(K, alloc, unit)
        for M in (1, 33):
            tern = C.ternary_case(M, N, K, sl)
            need = C.needle_case(M, N, K, sl)
            w_t, w_n = tern.w.to(DEV), need.w.to(DEV)
            for be in V1:
                out = poisoned_run(be, tern, 0, alloc, w_t)
                _collect(failures, out, tern, what(be))
                _collect(failures, run(be, need, w_dev=w_n, dev=DEV), need,
                         what(be))
            del w_t, w_n
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(1, 64, 2304), (33, 4096, 3584)])
def test_skinny_linear_empty_trailing_slices(M, N, K):
    """9 and 14 chunks over 8 slices of 2 leave 3 and 1 trailing slices
    without a K range; their slabs are never written and must not be
    summed.  (Before the launcher dropped them, this returned NaN.)"""
    be = V1[0]
    alloc = C.v1_splitk(N, K)
    sl = C.split_slices(K, alloc)
    assert alloc == 8 and len(sl) < alloc
    case = C.ternary_case(M, N, K, sl)
    out = poisoned_run(be, case, 0, alloc, case.w.to(DEV))
    print(f"M={M} N={N} K={K}: {int(out.isnan().sum())} NaN of {out.numel()}")
    C.assert_exact(out, case, what(be))


@pytest.mark.gpu
@pytest.mark.parametrize("be", BACKENDS, ids=_ids)
def test_scaled_exponents(be):
    M, N, K = 33, 192, 768
    case = C.scaled_case(M, N, K, slices_of(be, N, K))
    C.assert_exact(run(be, case, dev=DEV), case, what(be))


@pytest.mark.gpu
def test_v2_granule_ring_depths():
    """The ring depths docs/OPERATIONS.md offers beyond the defaults
    (6 plain M <= 32, 4 plain M > 32, 3 SiLU).  RLLI_SK2_G is read once
    per process: one fresh child per depth, none after a failure."""
    for g in (2, 6, 8):
        env = dict(os.environ, RLLI_SK2_G=str(g))
        r = subprocess.run(
            [sys.executable, "-m", "tests.gemm_exact_cases", "--v2-sweep"],
            cwd=REPO_ROOT, env=env, capture_output=True, text=True,
            timeout=120)
        assert r.returncode == 0, (
            f"RLLI_SK2_G={g}: exit {r.returncode}\n{r.stdout[-4000:]}\n"
            f"{r.stderr[-2000:]}")
        assert f"RLLI_SK2_G={g}: 64 runs, 0 wrong" in r.stdout, r.stdout
