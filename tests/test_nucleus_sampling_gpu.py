"""GPU tests for the fused sample_nucleus kernel and the engine's
device_sampling mode.  As in test_constrained_sampling_gpu.py there is no
tolerance: every z is bf16-exact (asserted), the host builds the kept set
in float64 from the definition and runs the EXISTING ops.sample on
``where(keep, z, -inf)``.  The inputs are chosen so that no nucleus cut is
borderline: no value's mass-strictly-above lies within a relative 1e-3 of
top_p * W (asserted), far above f32 exp error plus the 2^-32 quantisation
of 128k weights."""

import functools
import math

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.ops import ref
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 3
VOCABS = [8, 1003, 1004, 128256]
TEMPS = [0.0, 0.5, 1.0, 2.0]
KINDS = ["p0.1", "p0.5", "p0.9", "off", "pres", "freq", "both", "all",
         "hist300", "fullcap", "mixslot", "tie"]
LOGITS_SEED = 3017
NEG_INF = torch.tensor(float("-inf"), dtype=torch.float64)


_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)
_f32 = functools.partial(torch.tensor, dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _logits(V):
    # seeded so that no case has a borderline nucleus cut (see _oracle)
    g = torch.Generator().manual_seed(LOGITS_SEED + V)
    return (torch.randint(-32, 33, (B, V), generator=g) * 0.25).to(
        torch.bfloat16)


def _history(V, n, salt):      # a pool of 6 ids: small repeated counts
    g = torch.Generator().manual_seed(31 + salt)
    pool = torch.randint(0, V, (6,), generator=g)
    return pool[torch.randint(0, 6, (n,), generator=g)].tolist()


def _case(V, kind, combo):
    """One op call: the logits, the selected rows and everything per row."""
    lg = _logits(V)
    rows = [list(range(B)), [B - 1], [B - 1, 0, B - 1], []][combo]
    R = len(rows)
    c = dict(lg=lg, rows=rows, step=[0, 3, 0, 3][combo], cap=64,
             temps=[TEMPS[(i + combo) % 4] for i in range(B)],
             seeds=[11 + 7919 * i for i in range(B)],
             ks=[0] * R, ms=[0.0] * R, tps=[1.0] * R, pres=[0.0] * R,
             freq=[0.0] * R, biases=[[] for _ in range(R)],
             hists=[None] * R)
    T = [c["temps"][r] for r in rows]
    if kind.startswith("p0"):
        c["tps"] = [float(kind[1:])] * R
    if kind in ("pres", "both", "all", "mixslot", "fullcap"):
        c["pres"] = [0.5] * R
    if kind in ("freq", "both", "all", "hist300", "fullcap"):
        c["freq"] = [0.25] * R
    if kind in ("pres", "freq", "both", "all"):
        c["hists"] = [_history(V, 20, r + combo) for r in range(R)]
    if kind == "all":
        c["tps"] = [0.8] * R
        c["ks"] = [min(5 + 40 * r, V + 2) for r in range(R)]
        c["ms"] = [math.exp(-(r + 12.5) * 0.25 / T[r]) if T[r] > 0 else 0.5
                   for r in range(R)]          # cut 0.125 off the grid
        c["biases"] = [[[0, 1.5], [V // 2, -2.0], [V - 1, 0.75]]
                       if r % 2 == 0 else [] for r in range(R)]
    if kind == "hist300":
        # 8 - 0.25 * 300 = -67: still bf16-exact
        c["lg"] = lg = lg.clone()
        lg[:, V // 2] = 8.0
        c["hists"] = [[V // 2] * 300 + [0, V - 1] for _ in range(R)]
        c["cap"] = 320
        c["tps"] = [0.9] * R
    if kind == "fullcap":
        c["hists"] = [_history(V, 64, r + combo) for r in range(R)]
    if kind == "mixslot":
        c["hists"] = [_history(V, 20, r) if r % 2 == 0 else None
                      for r in range(R)]
        c["tps"] = [0.5] * R
    if kind == "tie":
        # 1, 3, 5 share the top value, 7 is the next lower one: the mass
        # crosses top_p inside the tie, all three stay and 7 goes
        c["lg"] = lg = torch.full((B, V), -8.0, dtype=torch.bfloat16)
        lg[:, [1, 3, 5]] = 4.0
        lg[:, 7] = 3.0
        c["tps"] = [0.5] * R
    return c


def _oracle(c):
    """float64 z and kept set of every selected row, from the definition."""
    lg, rows = c["lg"], c["rows"]
    V = lg.shape[1]
    z = lg[rows].double()
    keep = torch.ones(len(rows), V, dtype=torch.bool)
    for r in range(len(rows)):
        if c["hists"][r]:
            cnt = torch.bincount(torch.tensor(c["hists"][r]),
                                 minlength=V).double()
            z[r] -= torch.where(cnt > 0, c["pres"][r] + c["freq"][r] * cnt,
                                torch.zeros(V, dtype=torch.float64))
        for i, v in c["biases"][r]:
            z[r, i] += v
        T = c["temps"][rows[r]]
        if T <= 0:
            continue                          # filters are no-ops for greedy
        if 1 <= c["ks"][r] < V:
            keep[r] &= z[r] >= z[r].sort(descending=True).values[c["ks"][r] - 1]
        if c["ms"][r] > 0:
            cut = z[r].max() + T * math.log(c["ms"][r])
            assert (z[r] - cut).abs().min() > 0.12      # nobody borderline
            keep[r] &= z[r] >= cut
        tp = c["tps"][r]
        if 0 < tp < 1:
            w = torch.where(keep[r], torch.exp((z[r] - z[r].max()) / T),
                            torch.zeros(V, dtype=torch.float64))
            vals, inv = torch.unique(z[r], return_inverse=True)
            per = torch.zeros(len(vals), dtype=torch.float64).index_add_(
                0, inv, w)
            above = per.flip(0).cumsum(0).flip(0) - per
            target = tp * float(w.sum())
            assert ((above - target).abs() > 1e-3 * target).all()
            keep[r] &= above[inv] < target
    assert torch.equal(z.to(torch.bfloat16).double(), z)   # bf16-exact
    return z, keep


def _run(c, append=False, dev=DEV):
    """The op's arguments on ``dev`` (CPU: the reference) and its result."""
    rows, R = c["rows"], len(c["rows"])
    offs, ids, vals = [0], [], []
    for b in c["biases"]:
        ids += [i for i, _ in b]
        vals += [v for _, v in b]
        offs.append(len(ids))
    with_hist = [r for r in range(R) if c["hists"][r] is not None]
    slot_of = {r: len(with_hist) - 1 - j for j, r in enumerate(with_hist)}
    history = torch.zeros(len(with_hist), c["cap"], dtype=torch.int32)
    lens = [0] * len(with_hist)
    for r, s in slot_of.items():
        history[s, :len(c["hists"][r])] = torch.tensor(c["hists"][r])
        lens[s] = len(c["hists"][r])
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)     # noqa: E731
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    args = (c["lg"], i32(rows), f32(c["temps"]), torch.tensor(c["seeds"]),
            c["step"], i32(c["ks"]), f32(c["ms"]), f32(c["tps"]),
            f32(c["pres"]), f32(c["freq"]), i32(offs), i32(ids), f32(vals),
            i32([slot_of.get(r, -1) for r in range(R)]), history, i32(lens))
    args = tuple(a.to(dev) if torch.is_tensor(a) else a for a in args)
    return args, ops.sample_nucleus(*args, append)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VOCABS)
def test_matches_masked_sample(V, kind):
    for combo in range(4):
        c = _case(V, kind, combo)
        args, got1 = _run(c)
        lg_dev, history, hist_len = args[0], args[-2], args[-1]
        before = (lg_dev.clone(), history.clone(), hist_len.clone())
        got2 = ops.sample_nucleus(*args, False)
        torch.cuda.synchronize()
        rows, R = c["rows"], len(c["rows"])
        assert got1.shape == (R,) and got1.dtype == torch.int32
        assert torch.equal(got1, got2)        # repeated calls bit-identical
        assert all(torch.equal(a, b) for a, b in      # only the result written
                   zip(before, (lg_dev, history, hist_len)))
        if R == 0:
            continue
        z, keep = _oracle(c)
        rsel = torch.tensor(rows, device=DEV)
        want = ops.sample(torch.where(keep, z, NEG_INF).to(torch.bfloat16)
                          .to(DEV), args[2][rsel], args[3][rsel], c["step"])
        got = got1.tolist()
        assert got == want.tolist()
        for r in range(R):
            T = c["temps"][rows[r]]
            assert keep[r, got[r]]
            if T <= 0:                        # float64 arg-max, lowest index
                assert got[r] == int((z[r] == z[r].max()).nonzero()[0])
            if kind == "tie" and T in (0.5, 1.0):
                assert keep[r].nonzero().flatten().tolist() == [1, 3, 5]
        if kind == "off":
            # identity: no penalty, top_p off == the constrained sampler
            cs = ops.sample_constrained(*args[:7], *args[10:13])
            assert got == cs.tolist()


def test_append_and_second_call():
    """Greedy, frequency 0.25: token 2 (4.0) is taken and appended, which
    puts it at 3.75 behind token 6 (3.875); a slot at cap is left alone."""
    lg = torch.full((3, 16), -8.0, dtype=torch.bfloat16)
    lg[:, 2], lg[:, 6] = 4.0, 3.875
    c = dict(lg=lg, rows=[0, 1, 2], step=0, cap=4, temps=[0.0, 0.0, 1.0],
             seeds=[1, 2, 3], ks=[0] * 3, ms=[0.0] * 3, tps=[1.0] * 3,
             pres=[0.0] * 3, freq=[0.25] * 3, biases=[[], [], []],
             hists=[[9], [9, 9, 9, 9], None])
    args, got = _run(c, append=True)
    history, hist_len = args[-2], args[-1]        # slots: row 0 -> 1, 1 -> 0
    assert got.tolist()[:2] == [2, 2]
    assert hist_len.tolist() == [4, 2]
    assert history[1].tolist() == [9, 2, 0, 0]
    assert history[0].tolist() == [9, 9, 9, 9]
    again = ops.sample_nucleus(*args, True)
    assert again.tolist()[:2] == [6, 2]           # the full slot never saw 2
    assert hist_len.tolist() == [4, 3]
    assert history[1].tolist() == [9, 2, 6, 0]


def test_validation_errors():
    args, _ = _run(_case(1003, "both", 0))        # 3 rows, 3 slots
    limit = ops.sample_nucleus_max_history()
    assert limit == ref.NUCLEUS_MAX_HISTORY == 4096
    for pos, value in [
            (13, _i32([0, 0, 1])),                # one slot, two rows
            (13, _i32([0, 1, 3])),                # no such slot
            (14, torch.zeros(3, limit + 1, dtype=torch.int32, device=DEV)),
            (15, _i32([1, 2])), (13, _i32([0, 1])),          # lengths
            (7, _f32([0.5] * 2)), (8, _f32([0.5] * 4)), (9, _f32([0.5] * 2)),
            (7, _f32([0.5] * 3).double()), (14, args[14].long()),
            (0, torch.zeros(3, 262145, dtype=torch.bfloat16, device=DEV))]:
        bad = list(args)
        bad[pos] = value
        with pytest.raises(RuntimeError):
            ops.sample_nucleus(*bad, False)


def test_engine_device_sampling_eager_equals_graph(monkeypatch):
    """top_p, penalty, greedy and constrained rows in one batch: never the
    torch path, eager == graphed, device history == the row's output_ids."""
    from resilient_llm_amd.engine.graph import install_graph_runner
    sp = lambda **kw: SamplingParams(stop_on_eos=False, **kw)   # noqa: E731
    cfg = get_config("tiny-128")

    def run(graph):
        model = LlamaForCausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=3)
        e = LLMEngine(model, PagedKVCache.for_model(cfg, 256, device=DEV),
                      max_batch_size=8, device_sampling=True)
        if graph:
            install_graph_runner(e)
        monkeypatch.setattr(e, "_sample_torch", lambda *a, **k: pytest.fail(
            "_sample_torch reached"))
        e.add_request("p", list(range(5, 40)),
                      sp(max_tokens=10, temperature=0.9, seed=7, top_p=0.8))
        e.add_request("pen", list(range(9, 52)),
                      sp(max_tokens=12, presence_penalty=0.5,
                         frequency_penalty=0.25))
        e.add_request("g", list(range(3, 61)), sp(max_tokens=6))
        e.add_request("cs", list(range(20, 47)),
                      sp(max_tokens=10, temperature=1.1, seed=5, top_k=5))
        toks, flags, last = {}, [], None
        for _ in range(200):
            if not e.has_work():
                break
            for o in e.step():
                toks.setdefault(o.req_id, []).append(o.token_id)
            if e.running:
                flags.append(getattr(e, "_b_torch_sampling", False))
            if (any(s.req_id == "pen" for s in e.running)
                    and getattr(e, "_b_nuc_plan", None) is not None):
                last = e._b_nuc_plan
        assert not e.has_work() and not any(flags)
        assert not graph or e.stats["decode_steps"] > 0
        n = int(last[-1][0])
        assert last[-2][0, :n].tolist() == toks["pen"][:n] and n >= 11
        return toks

    eager = run(False)
    assert run(True) == eager
    assert [len(eager[k]) for k in ("p", "pen", "g", "cs")] == [10, 12, 6, 10]
