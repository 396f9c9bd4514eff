"""Engine-level logprobs on the CPU `tiny` model (vocab 512): the op is
called once per step for the rows that ask, with the step's FINAL
tokens; nothing happens for batches where nobody asks; records survive
speculative mode and live migration."""

import math

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config

_CFG = get_config("tiny")
_MODEL = LlamaForCausalLM(_CFG, device="cpu", dtype=torch.float32, seed=7)

PROMPT = list(range(9, 51))


def fresh_engine(**kw):
    kv = PagedKVCache.for_model(_CFG, 96, device="cpu")
    kv.k = kv.k.float()
    kv.v = kv.v.float()
    return LLMEngine(_MODEL, kv, max_batch_size=4, **kw)


def drain(e):
    outs = {}
    for _ in range(500):
        if not e.has_work():
            break
        for o in e.step():
            outs.setdefault(o.req_id, []).append(o)
    assert not e.has_work()
    return outs


def test_greedy_top5_consistent():
    e = fresh_engine()
    e.add_request("g", PROMPT, SamplingParams(max_tokens=10, logprobs=True,
                                              top_logprobs=5,
                                              stop_on_eos=False))
    outs = drain(e)["g"]
    assert len(outs) == 10
    for o in outs:
        assert len(o.top_logprobs) == 5
        tid, tlp = o.top_logprobs[0]
        assert tid == o.token_id and tlp == o.logprob
        vals = [v for _, v in o.top_logprobs]
        assert all(v <= 0 for v in vals)
        assert vals == sorted(vals, reverse=True)
        assert sum(math.exp(v) for v in vals) <= 1 + 1e-4


@pytest.mark.parametrize("kw", [
    dict(),                                              # greedy
    dict(temperature=0.8, seed=99),                      # sampled
    dict(temperature=0.9, top_p=0.8, seed=7),            # top-p override
])
def test_tokens_identical_with_and_without_logprobs(kw):
    def run(on):
        e = fresh_engine()
        e.add_request("r", PROMPT, SamplingParams(
            max_tokens=12, stop_on_eos=False, logprobs=on,
            top_logprobs=4 if on else 0, **kw))
        return drain(e)["r"]
    off, on = run(False), run(True)
    assert [o.token_id for o in on] == [o.token_id for o in off]
    assert all(o.logprob is None and o.top_logprobs is None for o in off)
    assert all(o.logprob is not None and len(o.top_logprobs) == 4
               for o in on)


def test_only_requesting_rows_pay(monkeypatch):
    calls = []
    real = ops.token_logprobs

    def counting(logits, rows, tokens, k):
        calls.append((rows.tolist(), k))
        return real(logits, rows, tokens, k)

    monkeypatch.setattr(ops, "token_logprobs", counting)

    def batch(ask):
        e = fresh_engine()
        e.add_request("a", PROMPT, SamplingParams(max_tokens=6,
                                                  stop_on_eos=False))
        e.add_request("b", PROMPT[3:], SamplingParams(
            max_tokens=6, stop_on_eos=False, logprobs=ask,
            top_logprobs=2 if ask else 0))
        e.add_request("c", PROMPT[5:], SamplingParams(
            max_tokens=6, temperature=0.7, seed=3, stop_on_eos=False))
        return drain(e)

    outs = batch(False)
    assert calls == []                   # nobody asks: the op never runs
    assert all(o.logprob is None for v in outs.values() for o in v)

    outs = batch(True)
    assert len(calls) == 6               # once per step, not per row
    assert all(rows == [1] and k == 2 for rows, k in calls)
    for rid in ("a", "c"):
        assert all(o.logprob is None and o.top_logprobs is None
                   for o in outs[rid])
    assert all(o.logprob is not None and len(o.top_logprobs) == 2
               for o in outs["b"])


def test_row_index_upload_is_per_batch_not_per_step(monkeypatch):
    """The requesting-row tensor is a host->device upload (a stream
    synchronize on the GPU): it is built when the batch composition
    changes, never once per decode step."""
    e = fresh_engine()
    calls = []
    real = e._lp_plan
    monkeypatch.setattr(e, "_lp_plan",
                        lambda seqs: calls.append(len(seqs)) or real(seqs))
    e.add_request("r", PROMPT, SamplingParams(max_tokens=12, logprobs=True,
                                              top_logprobs=2,
                                              stop_on_eos=False))
    outs = drain(e)["r"]
    assert len(outs) == 12 and all(o.logprob is not None for o in outs)
    assert e.stats["decode_steps"] == 11
    assert len(calls) == 2          # the prefill step + ONE batch rebuild


def test_override_rows_report_the_final_token(monkeypatch):
    """top-p + penalty: the reported logprob is the float64 log-softmax
    of the RAW logits row at the token the override finally chose."""
    e = fresh_engine()
    captured = []
    real = e._sample

    def wrapped(logits, seqs):
        toks = real(logits, seqs)
        captured.append((logits.detach().clone(), list(toks)))
        return toks

    monkeypatch.setattr(e, "_sample", wrapped)
    e.add_request("p", PROMPT, SamplingParams(
        max_tokens=10, temperature=0.9, top_p=0.7, presence_penalty=0.8,
        frequency_penalty=0.3, seed=11, stop_on_eos=False, logprobs=True,
        top_logprobs=3))
    outs = drain(e)["p"]
    assert len(outs) == len(captured) == 10
    for o, (logits, toks) in zip(outs, captured):
        assert toks == [o.token_id]
        x = logits[0].double()
        want = (x - torch.logsumexp(x, 0))[o.token_id].item()
        assert abs(o.logprob - want) <= 1e-4
        assert o.logprob <= o.top_logprobs[0][1]


def test_spec_lookup_still_one_record_per_token():
    e = fresh_engine(spec_lookup=4)
    # repetitive prompt so prompt-lookup WOULD propose if it were eligible
    e.add_request("s", [5, 6, 7, 8] * 8, SamplingParams(
        max_tokens=12, stop_on_eos=False, logprobs=True, top_logprobs=1))
    outs = drain(e)["s"]
    assert len(outs) == 12
    assert all(o.logprob is not None and len(o.top_logprobs) == 1
               for o in outs)
    assert e.stats.get("spec_steps", 0) == 0


def test_top_logprobs_out_of_range_rejected():
    e = fresh_engine()
    with pytest.raises(ValueError):
        e.add_request("x", PROMPT, SamplingParams(logprobs=True,
                                                  top_logprobs=21))


def _records(outs):
    return [[o.logprob, [[t, v] for t, v in o.top_logprobs]] for o in outs]


def test_migration_carries_records():
    params = lambda: SamplingParams(max_tokens=14, temperature=0.8,  # noqa: E731
                                    seed=99, stop_on_eos=False,
                                    logprobs=True, top_logprobs=3)
    ref = fresh_engine()
    ref.add_request("m", PROMPT, params())
    want = drain(ref)["m"]

    src, dst = fresh_engine(), fresh_engine()
    src.add_request("m", PROMPT, params())
    got = []
    for _ in range(6):
        got.extend(src.step())
    assert 0 < len(got) < 14
    src.request_extract("m")
    src.step()
    state = src.take_extracted("m")
    assert state is not None and state["kv"] is not None
    # plain lists / floats / ints only, one record per output token
    assert state["output_logprobs"] == _records(got)
    assert len(state["output_logprobs"]) == len(state["output_ids"])
    assert state["params"]["logprobs"] is True
    assert state["params"]["top_logprobs"] == 3

    dst.queue_adopt(state)
    tail = drain(dst)["m"]
    assert dst.take_adopt_result("m") == "ok"
    allo = got + tail
    assert [o.token_id for o in allo] == [o.token_id for o in want]
    for a, w in zip(allo, want):
        assert abs(a.logprob - w.logprob) <= 1e-4
        assert [t for t, _ in a.top_logprobs] == [t for t, _ in w.top_logprobs]
        for (_, av), (_, wv) in zip(a.top_logprobs, w.top_logprobs):
            assert abs(av - wv) <= 1e-4


def test_adopt_accepts_blob_without_records():
    src, dst = fresh_engine(), fresh_engine()
    src.add_request("o", PROMPT, SamplingParams(max_tokens=8,
                                                stop_on_eos=False))
    for _ in range(4):
        src.step()
    src.request_extract("o")
    src.step()
    state = src.take_extracted("o")
    state.pop("output_logprobs")         # blob from before this field
    state["params"].pop("logprobs")
    state["params"].pop("top_logprobs")
    dst.queue_adopt(state)
    tail = drain(dst)["o"]
    assert dst.take_adopt_result("o") == "ok"
    assert len(state["output_ids"]) + len(tail) == 8
