"""GPU tests for the fused sample_constrained kernel (logit_bias, top_k,
min_p) and its engine wiring.

The kernel is checked WITHOUT a tolerance.  Logits are multiples of 0.25
in [-8, 8] and biases multiples of 0.25 in [-8, 8], so every biased
logit z is exactly representable in bf16 (|z| <= 16 needs 7 significand
bits).  The host builds the kept set in float64 from the definition,
writes ``where(keep, z, -inf)`` as bf16 and runs the EXISTING ops.sample
on it: sample_constrained must return the same tokens, twice in a row.
min_p cuts are placed 0.125 away from every grid value (asserted), far
outside fp32 error of ``z_max + T*ln(m)``.
"""

import functools
import math

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 8), (3, 512), (3, 1003), (3, 1004), (5, 128256)]
TEMPS = [0.0, 0.5, 1.0, 2.0]


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _f32(x):
    return torch.tensor(x, dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _logits(B, V):
    g = torch.Generator().manual_seed(1000 * B + V)
    cpu = (torch.randint(-32, 33, (B, V), generator=g) * 0.25).to(
        torch.bfloat16)
    return cpu, cpu.to(DEV)


def _bias_list(V, n, salt):
    """n distinct ascending ids (0 and V-1 among them when n >= 2) with
    biases that are multiples of 0.25 in [-8, 8]."""
    n = min(n, V)
    g = torch.Generator().manual_seed(77 + salt)
    if n == 1:
        ids = [V - 1 if salt % 2 else 0]
    else:
        mid = (torch.randperm(V - 2, generator=g)[:n - 2] + 1).tolist()
        ids = sorted([0, V - 1] + mid)
    vals = (torch.randint(-32, 33, (n,), generator=g) * 0.25).tolist()
    return [[i, v] for i, v in zip(ids, vals)]


def _csr(biases):
    offs, ids, vals = [0], [], []
    for b in biases:
        ids += [int(i) for i, _ in b]
        vals += [float(v) for _, v in b]
        offs.append(len(ids))
    return _i32(offs), _i32(ids), _f32(vals)


def _min_p(T, n):
    # cut = z_max - (n + 0.5) * 0.25: 0.125 from every grid value
    return math.exp(-(n + 0.5) * 0.25 / T) if T > 0 else 0.5


def _check(lg_cpu, lg_dev, rows, temps, seeds, step, ks, ms, biases):
    """Run the op on ``rows`` and compare with the masked-copy oracle."""
    B, V = lg_cpu.shape
    R = len(rows)
    offs, ids, vals = _csr(biases)
    temps_d, seeds_d = _f32(temps), torch.tensor(seeds, dtype=torch.int64,
                                                 device=DEV)
    args = (lg_dev, _i32(rows), temps_d, seeds_d, step, _i32(ks), _f32(ms),
            offs, ids, vals)
    before = lg_dev.clone()
    got1 = ops.sample_constrained(*args)
    got2 = ops.sample_constrained(*args)
    torch.cuda.synchronize()
    assert got1.shape == (R,) and got1.dtype == torch.int32
    assert torch.equal(got1, got2)            # repeated calls bit-identical
    assert torch.equal(lg_dev, before)        # the logits are only read
    if R == 0:
        return got1
    z = lg_cpu[rows].double()
    for r, b in enumerate(biases):
        for i, v in b:
            z[r, i] += v
    assert torch.equal(z.to(torch.bfloat16).double(), z)   # bf16-exact
    keep = torch.ones(R, V, dtype=torch.bool)
    for r in range(R):
        T = temps[rows[r]]
        if T <= 0:
            continue                          # filters are no-ops for greedy
        if 1 <= ks[r] < V:
            kth = z[r].sort(descending=True).values[ks[r] - 1]
            keep[r] &= z[r] >= kth
        if ms[r] > 0:
            cut = z[r].max() + T * math.log(ms[r])
            assert (z[r] - cut).abs().min() > 0.12      # nobody borderline
            keep[r] &= z[r] >= cut
    masked = torch.where(keep, z, torch.tensor(float("-inf"),
                                               dtype=torch.float64))
    want = ops.sample(masked.to(torch.bfloat16).to(DEV),
                      temps_d[torch.tensor(rows, device=DEV)],
                      seeds_d[torch.tensor(rows, device=DEV)], step)
    assert got1.tolist() == want.tolist()
    got = got1.tolist()
    for r in range(R):
        assert keep[r, got[r]]
        if temps[rows[r]] <= 0:               # float64 arg-max, lowest index
            assert got[r] == int((z[r] == z[r].max()).nonzero()[0])
    return got1


def _row_sets(B):
    sub = [B - 1] if B > 1 else [0]
    rep = [B - 1, 0, B - 1] if B > 1 else [0, 0]
    return [list(range(B)), sub, rep, list(range(B))]


KINDS = ["none", "k1", "k5", "kV-1", "kV", "kV+7", "min_p", "bias1",
         "bias300", "all", "tie"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,V", SHAPES)
def test_matches_masked_sample(B, V, kind):
    lg_cpu, lg_dev = _logits(B, V)
    if kind == "tie":
        # three tokens share the row maximum: k = 2 must keep all three
        lg_cpu = lg_cpu.clone()
        lg_cpu[:, [1, 3, 5]] = 9.0
        lg_dev = lg_cpu.to(DEV)
    seeds = [11 + 7919 * i for i in range(B)]
    for combo, rows in enumerate(_row_sets(B)):
        step = [0, 3, 0, 3][combo]
        temps = [TEMPS[(i + combo) % 4] for i in range(B)]
        R = len(rows)
        ks, ms, biases = [0] * R, [0.0] * R, [[] for _ in range(R)]
        if kind.startswith("k"):
            ks = [{"k1": 1, "k5": 5, "kV-1": V - 1, "kV": V,
                   "kV+7": V + 7}[kind]] * R
        if kind == "tie":
            ks = [2] * R
        if kind in ("min_p", "all"):
            ms = [_min_p(temps[rows[r]], 3 + r) for r in range(R)]
        if kind == "bias1":
            biases = [_bias_list(V, 1, r + combo) for r in range(R)]
        if kind == "bias300":
            biases = [_bias_list(V, 300, r + combo) for r in range(R)]
        if kind == "all":
            ks = [min(5 + 40 * r, V + 2) for r in range(R)]
            # rows with and without a bias in one CSR list
            biases = [_bias_list(V, 16, r + combo) if r % 2 == 0 else []
                      for r in range(R)]
        got = _check(lg_cpu, lg_dev, rows, temps, seeds, step, ks, ms, biases)
        if kind == "none":
            # identity: no constraint == the plain sampler's row
            plain = ops.sample(lg_dev, _f32(temps),
                               torch.tensor(seeds, dtype=torch.int64,
                                            device=DEV), step)
            assert got.tolist() == [plain.tolist()[r] for r in rows]
        if kind == "tie":
            for r in range(R):
                if temps[rows[r]] > 0:
                    assert got[r].item() in (1, 3, 5)


def test_empty_selection():
    lg_cpu, lg_dev = _logits(3, 512)
    got = _check(lg_cpu, lg_dev, [], [1.0] * 3, [1, 2, 3], 0, [], [], [])
    assert got.numel() == 0


def test_largest_supported_vocab():
    V = 262144
    lg = torch.zeros(1, V, dtype=torch.bfloat16, device=DEV)
    offs, ids, vals = _csr([[[V - 1, 4.0]]])
    for T in (0.0, 1.0):
        got = ops.sample_constrained(
            lg, _i32([0]), _f32([T]), torch.tensor([5], device=DEV), 0,
            _i32([1]), _f32([0.0]), offs, ids, vals)
        assert got.tolist() == [V - 1]


def _repeat_rows(V=64, N=4096):
    g = torch.Generator().manual_seed(5)
    row = (torch.randint(-8, 9, (V,), generator=g) * 0.25)
    lg = row.to(torch.bfloat16).repeat(N, 1).contiguous().to(DEV)
    seeds = torch.arange(N, dtype=torch.int64, device=DEV) * 104729 + 13
    return row.double(), lg, seeds, N


def _run_repeat(lg, seeds, N, k, bias):
    offs, ids, vals = _csr([bias] * N)
    return ops.sample_constrained(
        lg, torch.arange(N, dtype=torch.int32, device=DEV),
        torch.ones(N, device=DEV), seeds, 0, _i32([k] * N),
        _f32([0.0] * N), offs, ids, vals).cpu()


def test_ban_and_force():
    row, lg, seeds, N = _repeat_rows()
    top = int(row.argmax())
    plain = _run_repeat(lg, seeds, N, 0, [])
    assert (plain == top).any()               # it does get drawn unbanned
    banned = _run_repeat(lg, seeds, N, 0, [[top, -100.0]])
    assert not (banned == top).any()
    forced = _run_repeat(lg, seeds, N, 0, [[17, 100.0]])
    assert (forced == 17).all()


def test_top_k_distribution():
    """k = 4 on distinct top values: the four survivors' frequencies over
    4096 independent seeds lie within 5 sigma of softmax over the kept
    set, and nothing else is drawn."""
    row, lg, seeds, N = _repeat_rows()
    lg = lg.clone()
    tops = {3: 4.0, 20: 3.5, 41: 3.0, 60: 2.5}          # the rest is <= 2
    for i, v in tops.items():
        lg[:, i] = v
    got = _run_repeat(lg, seeds, N, 4, [])
    p = torch.softmax(torch.tensor(list(tops.values()), dtype=torch.float64),
                      0).tolist()
    counts = {i: int((got == i).sum()) for i in tops}
    assert sum(counts.values()) == N
    for (i, _), pi in zip(tops.items(), p):
        sigma = math.sqrt(pi * (1 - pi) / N)
        print(i, counts[i] / N, pi, sigma)
        assert abs(counts[i] / N - pi) <= 5 * sigma


def test_validation_errors():
    _, lg = _logits(3, 512)
    seeds = torch.tensor([1, 2, 3], dtype=torch.int64, device=DEV)
    temps = _f32([1.0] * 3)

    def call(logits=lg, rows=None, temps=temps, seeds=seeds, top_k=None,
             min_p=None, offs=None, ids=None, vals=None):
        return ops.sample_constrained(
            logits, _i32([0, 1]) if rows is None else rows, temps, seeds, 0,
            _i32([0, 0]) if top_k is None else top_k,
            _f32([0.0, 0.0]) if min_p is None else min_p,
            _i32([0, 1, 1]) if offs is None else offs,
            _i32([4]) if ids is None else ids,
            _f32([1.0]) if vals is None else vals)

    assert call().shape == (2,)
    bad = [dict(logits=lg.float()),
           dict(rows=torch.tensor([0, 1], device=DEV)),            # int64
           dict(temps=temps.double()),
           dict(seeds=seeds.int()),
           dict(top_k=_f32([0.0, 0.0])),
           dict(min_p=_i32([0, 0])),
           dict(offs=torch.tensor([0, 1, 1], device=DEV)),
           dict(ids=torch.tensor([4], device=DEV)),
           dict(vals=torch.tensor([1.0], dtype=torch.float64, device=DEV)),
           dict(top_k=_i32([0])),                                  # lengths
           dict(min_p=_f32([0.0, 0.0, 0.0])),
           dict(offs=_i32([0, 1])),
           dict(ids=_i32([4, 5])),
           dict(temps=_f32([1.0] * 2)),
           dict(logits=torch.zeros(3, 262145, dtype=torch.bfloat16,
                                   device=DEV))]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)


# ------------------------------------------------------------ engine
def _make_engine(graph, seed=3):
    from resilient_llm_amd.engine.graph import install_graph_runner
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=seed)
    kv = PagedKVCache.for_model(cfg, 256, device=DEV)
    e = LLMEngine(model, kv, max_batch_size=8)
    if graph:
        install_graph_runner(e)
    return e


def _drain(engine):
    outs = {}
    for _ in range(1000):
        if not engine.has_work():
            break
        for o in engine.step():
            outs.setdefault(o.req_id, []).append(o)
    assert not engine.has_work()
    return outs


def _toks(outs):
    return {k: [o.token_id for o in v] for k, v in outs.items()}


def test_engine_graph_constrained_rows(monkeypatch):
    """One graphed batch: a sampled top_k/min_p row, a greedy row that
    bans its own first token, a greedy row forced onto one token, a
    sampled top_k = 1 row with logprobs and a plain request.  Every
    decode step is a graph replay followed by one device op — the torch
    path is never reached — and the tokens equal the eager engine's."""
    P_BAN, P_PLAIN = list(range(9, 52)), list(range(3, 61))
    sp = lambda **kw: SamplingParams(stop_on_eos=False, **kw)   # noqa: E731
    FORCED = 77

    base = _make_engine(graph=False)
    base.add_request("ban", P_BAN, sp(max_tokens=1))
    first = _toks(_drain(base))["ban"][0]

    def load(e, everyone=True):
        e.add_request("n", P_PLAIN, sp(max_tokens=5))
        if not everyone:
            return
        e.add_request("s", list(range(5, 40)),
                      sp(max_tokens=8, temperature=0.9, seed=7, top_k=5,
                         min_p=0.05))
        e.add_request("ban", P_BAN,
                      sp(max_tokens=8, logit_bias=[[first, -100.0]]))
        e.add_request("force", list(range(20, 47)),
                      sp(max_tokens=8, logit_bias=[[FORCED, 100.0]]))
        e.add_request("k1", list(range(30, 70)),
                      sp(max_tokens=8, temperature=1.3, seed=11, top_k=1,
                         logprobs=True, top_logprobs=2))

    def no_torch(*a, **k):
        raise AssertionError("_sample_torch reached")

    eager = _make_engine(graph=False)
    monkeypatch.setattr(eager, "_sample_torch", no_torch)
    load(eager)
    want = _toks(_drain(eager))

    alone = _make_engine(graph=True)
    load(alone, everyone=False)
    plain_alone = _toks(_drain(alone))["n"]

    g = _make_engine(graph=True)
    monkeypatch.setattr(g, "_sample_torch", no_torch)
    load(g)
    replays, torch_flags = [], []
    real_step = g.graph_runner.step

    def counted_step():
        replays.append(1)
        torch_flags.append(g._b_torch_sampling)
        return real_step()

    g.graph_runner.step = counted_step
    outs = _drain(g)
    got = _toks(outs)
    assert replays and len(replays) == g.stats["decode_steps"]
    assert not any(torch_flags)
    assert got["n"] == plain_alone
    assert got == want
    assert first not in got["ban"] and len(got["ban"]) == 8
    assert got["force"] == [FORCED] * 8
    assert len(got["s"]) == 8
    for o in outs["k1"]:
        assert o.logprob == o.top_logprobs[0][1]
