"""GPU tests for the fused token_logprobs kernel and its engine wiring.

Reference: float64 log-softmax on the CPU over the exact bf16 values,
ordered with a stable descending sort (value descending, index
ascending).  ids must match exactly (selection compares bf16 values
only); values within 1e-3 absolute: fp32 accumulation over 128k terms is
~1.4e-5 from float64 with torch's own fp32 log_softmax, the fast exp/log
intrinsics add ~1e-6 relative, so 1e-3 is ~70x that and still 15x finer
than one bf16 step at logit magnitude 4.
"""

import functools
import math

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config

pytestmark = pytest.mark.gpu

TOL = 1e-3
V_LLAMA = 128256


@functools.lru_cache(maxsize=None)
def _seeded(B, V):
    g = torch.Generator().manual_seed(1000 * B + V)
    return (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16)


def _reference(logits_cpu, rows, tokens, k):
    x = logits_cpu[rows].double()
    lp = x - torch.logsumexp(x, dim=-1, keepdim=True)
    chosen = lp.gather(1, torch.tensor(tokens).unsqueeze(1)).squeeze(1)
    vals, ids = torch.sort(lp, dim=-1, descending=True, stable=True)
    return chosen, vals[:, :k], ids[:, :k]


def _run_and_check(logits_cpu, rows, k, seed=0):
    V = logits_cpu.shape[1]
    g = torch.Generator().manual_seed(seed + 17)
    tokens = torch.randint(0, V, (len(rows),), generator=g).tolist()
    dev = logits_cpu.to("cuda:0")
    rows_d = torch.tensor(rows, dtype=torch.int32, device="cuda:0")
    toks_d = torch.tensor(tokens, dtype=torch.int32, device="cuda:0")
    c1, v1, i1 = ops.token_logprobs(dev, rows_d, toks_d, k)
    c2, v2, i2 = ops.token_logprobs(dev, rows_d, toks_d, k)
    torch.cuda.synchronize()
    assert c1.shape == (len(rows),) and c1.dtype == torch.float32
    assert v1.shape == (len(rows), k) and v1.dtype == torch.float32
    assert i1.shape == (len(rows), k) and i1.dtype == torch.int32
    # repeated calls are bit-identical (no atomics, fixed reduction order)
    assert torch.equal(c1, c2) and torch.equal(v1, v2) and torch.equal(i1, i2)
    want_c, want_v, want_i = _reference(logits_cpu, rows, tokens, k)
    err_c = (c1.cpu().double() - want_c).abs().max().item() if rows else 0.0
    err_v = (v1.cpu().double() - want_v).abs().max().item() \
        if rows and k else 0.0
    print(f"token_logprobs B={logits_cpu.shape[0]} V={V} R={len(rows)} "
          f"k={k}: max|err| chosen={err_c:.3e} top={err_v:.3e}")
    assert torch.equal(i1.cpu().long(), want_i), "top ids / tie order differ"
    assert err_c <= TOL
    assert err_v <= TOL
    return c1, v1, i1


CASES = [
    (1, 8, [0], 8),
    (3, 512, [2, 0], 20),
    (4, 1000, None, 5),
    (3, 1003, None, 20),            # misaligned rows plus a % 8 tail
    # row bases 0 / 6 / 12 bytes past 16-byte alignment above (16-, 2- and
    # 4-byte load paths); 1004 puts row 1 at 8 (the 8-byte path)
    (3, 1004, None, 20),
    (5, V_LLAMA, [4, 1], 1),
    (5, V_LLAMA, [4, 1, 4], 0),
    (64, V_LLAMA, None, 20),
    # more than 512 merge candidates (n_split * k): phase B leaves its
    # register path; odd vocab so rows 1.. are misaligned too
    (2, 27 * 8192 + 3, None, 20),
]


@pytest.mark.parametrize("B,V,rows,k", CASES)
def test_kernel_matches_float64(B, V, rows, k):
    rows = list(range(B)) if rows is None else rows
    _run_and_check(_seeded(B, V), rows, k)


def test_kernel_empty_selection():
    dev = _seeded(3, 512).to("cuda:0")
    e = torch.empty(0, dtype=torch.int32, device="cuda:0")
    c, v, i = ops.token_logprobs(dev, e, e, 5)
    assert c.shape == (0,) and v.shape == (0, 5) and i.shape == (0, 5)


def test_kernel_validation():
    dev = _seeded(3, 512).to("cuda:0")
    r = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    with pytest.raises(RuntimeError):
        ops.token_logprobs(dev, r, r, 21)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(dev, r, r, -1)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(dev, r, r[:1], 1)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(dev, r.long(), r, 1)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(dev.float(), r, r, 1)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(_seeded(1, 8).to("cuda:0"), r[:1], r[:1], 9)


def test_kernel_crafted_rows():
    V = V_LLAMA
    base = _seeded(2, V).clamp(max=30.0)
    equal = torch.full((V,), 1.5, dtype=torch.bfloat16)
    last = base[0].clone()
    last[V - 1] = 64.0
    first = torch.full((V,), -1e4, dtype=torch.bfloat16)
    first[0] = 4.0
    straddle = base[1].clone()
    pos = []
    for i in range(1, 11):                      # split boundaries at i*V/16
        pos += [i * (V // 16) - 1, i * (V // 16) + 1]
    for j, p in enumerate(pos):
        straddle[p] = 50.0 + (j % 3)            # ties ACROSS chunks
    logits = torch.stack([equal, last, first, straddle])
    _, v, i = _run_and_check(logits, [0, 1, 2, 3], 20)
    i = i.cpu().tolist()
    assert i[0] == list(range(20))
    assert abs(v[0, 0].item() + math.log(V)) <= TOL
    assert i[1][0] == V - 1
    assert i[2] == list(range(20))
    assert sorted(i[3]) == sorted(pos)


# ------------------------------------------------------------ engine
def _make_engine(seed=3):
    from resilient_llm_amd.engine.graph import install_graph_runner
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device="cuda:0", dtype=torch.bfloat16,
                             seed=seed)
    kv = PagedKVCache.for_model(cfg, 256, device="cuda:0")
    e = LLMEngine(model, kv, max_batch_size=8)
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


def test_engine_graph_logprobs():
    """One graphed batch: greedy+logprobs, top-p+logprobs and a plain
    request.  Tokens equal a run with logprobs off; greedy chosen ==
    top-1; sampled chosen <= top-1; the plain request carries None."""
    def load(e, on):
        e.add_request("g", list(range(5, 40)),
                      SamplingParams(max_tokens=8, logprobs=on,
                                     top_logprobs=5 if on else 0))
        e.add_request("p", list(range(9, 52)),
                      SamplingParams(max_tokens=8, temperature=0.9,
                                     top_p=0.8, seed=7, logprobs=on,
                                     top_logprobs=3 if on else 0))
        e.add_request("n", list(range(3, 61)), SamplingParams(max_tokens=8))

    off = _make_engine()
    load(off, False)
    want = {k: [o.token_id for o in v] for k, v in _drain(off).items()}
    on = _make_engine()
    load(on, True)
    replays = []
    real_step = on.graph_runner.step
    on.graph_runner.step = lambda: replays.append(1) or real_step()
    got = _drain(on)
    # every decode step really was a steady graph replay (not the eager
    # branch): the wiring after gr.step() / override_tokens is what ran
    assert replays and len(replays) == on.stats["decode_steps"]
    assert {k: [o.token_id for o in v] for k, v in got.items()} == want
    for o in got["g"]:
        assert len(o.top_logprobs) == 5
        assert o.top_logprobs[0][0] == o.token_id
        assert o.top_logprobs[0][1] == o.logprob
        assert o.logprob <= 0
    for o in got["p"]:
        assert len(o.top_logprobs) == 3
        assert o.logprob <= o.top_logprobs[0][1] <= 0
        if o.top_logprobs[0][0] == o.token_id:
            assert o.logprob == o.top_logprobs[0][1]
    for o in got["n"]:
        assert o.logprob is None and o.top_logprobs is None
    # the logprobs-off engine never allocated logprob landing buffers
    assert off._pinned_lp is None
