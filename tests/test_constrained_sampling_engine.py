"""Engine-level logit_bias / top_k / min_p on the CPU `tiny` model
(vocab 512): constrained rows are served by one ops.sample_constrained
call per step from a per-batch plan, never by the torch path; the
per-(request, output index) seed contract holds alone, in a batch and
across migration."""

import dataclasses

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
            outs.setdefault(o.req_id, []).append(o.token_id)
    assert not e.has_work()
    return outs


def sp(**kw):
    kw.setdefault("max_tokens", 10)
    kw.setdefault("stop_on_eos", False)
    return SamplingParams(**kw)


CONSTRAINED = dict(temperature=0.9, seed=21, top_k=6, min_p=0.02,
                   logit_bias=[[3, -100.0], [77, 2.5]])


def test_properties():
    assert not SamplingParams().needs_constrained_sampling
    assert not SamplingParams(top_k=5, min_p=0.1).needs_constrained_sampling
    assert SamplingParams(temperature=1.0, top_k=5).needs_constrained_sampling
    assert SamplingParams(temperature=1.0, min_p=0.1).needs_constrained_sampling
    assert SamplingParams(logit_bias=[[1, 2.0]]).needs_constrained_sampling
    assert not SamplingParams(logit_bias=[]).needs_constrained_sampling
    p = SamplingParams(temperature=1.0, top_k=5, logit_bias=[[1, 2.0]])
    assert not p.needs_torch_sampling        # its meaning did not change
    assert SamplingParams(temperature=1.0, top_p=0.5,
                          top_k=5).needs_torch_sampling


def test_asdict_round_trip():
    p = sp(**CONSTRAINED)
    d = dataclasses.asdict(p)
    assert d["logit_bias"] == [[3, -100.0], [77, 2.5]]
    assert d["top_k"] == 6 and d["min_p"] == 0.02
    assert SamplingParams(**d) == p


@pytest.mark.parametrize("kw", [
    dict(top_k=-1),
    dict(min_p=-0.1),
    dict(min_p=1.5),
    dict(logit_bias=[[i, 1.0] for i in range(301)]),
    dict(logit_bias=[[4, 1.0], [4, 2.0]]),
    dict(logit_bias=[[-1, 1.0]]),
    dict(logit_bias=[[_CFG.vocab_size, 1.0]]),
    dict(logit_bias=[[4, 100.5]]),
    dict(logit_bias=[[4, -101.0]]),
])
def test_add_request_rejects(kw):
    e = fresh_engine()
    with pytest.raises(ValueError):
        e.add_request("x", PROMPT, sp(**kw))
    assert not e.has_work()


def test_add_request_accepts_limits():
    e = fresh_engine()
    e.add_request("x", PROMPT, sp(top_k=10 ** 6, min_p=1.0, max_tokens=2,
                                  logit_bias=[[i, -100.0] for i in range(300)]))
    assert len(drain(e)["x"]) == 2


def test_identical_alone_and_in_a_batch(monkeypatch):
    e = fresh_engine()
    monkeypatch.setattr(e, "_sample_torch", None)      # must not be reached
    e.add_request("c", PROMPT, sp(**CONSTRAINED))
    alone = drain(e)["c"]
    assert 3 not in alone                    # banned
    assert len(set(alone)) > 1

    e = fresh_engine()
    monkeypatch.setattr(e, "_sample_torch", None)
    e.add_request("a", PROMPT[2:], sp(temperature=0.7, seed=5))
    e.add_request("c", PROMPT, sp(**CONSTRAINED))
    e.add_request("g", PROMPT[4:], sp(max_tokens=4))   # leaves: a rebuild
    assert drain(e)["c"] == alone


def test_neighbours_unaffected_by_the_feature():
    def run(with_feature):
        e = fresh_engine()
        e.add_request("plain", PROMPT[2:], sp(temperature=0.7, seed=5))
        e.add_request("greedy", PROMPT[4:], sp())
        e.add_request("nb", PROMPT, sp(**CONSTRAINED) if with_feature
                      else sp(temperature=0.9, seed=21))
        return drain(e)
    a, b = run(False), run(True)
    assert a["plain"] == b["plain"] and a["greedy"] == b["greedy"]
    assert a["nb"] != b["nb"]


def test_greedy_ban_and_force():
    e = fresh_engine()
    e.add_request("g", PROMPT, sp())
    base = drain(e)["g"]
    e = fresh_engine()
    e.add_request("ban", PROMPT, sp(logit_bias=[[base[0], -100.0]]))
    e.add_request("force", PROMPT, sp(logit_bias=[[123, 100.0]]))
    # greedy rows: top_k / min_p change nothing
    e.add_request("noop", PROMPT, sp(top_k=1, min_p=0.9))
    out = drain(e)
    assert base[0] not in out["ban"]
    assert out["force"] == [123] * 10
    assert out["noop"] == base


def test_plan_is_per_batch_not_per_step(monkeypatch):
    """The plan's tensors are host->device uploads: built when the batch
    composition changes, never once per decode step; the op runs once
    per step for the constrained rows only."""
    e = fresh_engine()
    plans, calls = [], []
    real_plan, real_op = e._cs_plan, ops.sample_constrained
    monkeypatch.setattr(e, "_cs_plan",
                        lambda seqs: plans.append(len(seqs)) or real_plan(seqs))

    def counting(logits, rows, *a):
        calls.append(rows.tolist())
        return real_op(logits, rows, *a)

    monkeypatch.setattr(ops, "sample_constrained", counting)
    monkeypatch.setattr(e, "_sample_torch", None)
    e.add_request("p", PROMPT[1:], sp(max_tokens=12))
    e.add_request("c", PROMPT, sp(**{**CONSTRAINED, "max_tokens": 12}))
    out = drain(e)
    assert len(out["c"]) == 12
    assert e.stats["decode_steps"] == 11
    assert len(plans) == 2          # the prefill step + ONE batch rebuild
    assert calls == [[1]] * 12      # once per step, the constrained row only
    assert e._b_torch_sampling is False


def test_batches_without_the_feature_touch_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("sample_constrained called")
    monkeypatch.setattr(ops, "sample_constrained", boom)
    e = fresh_engine()
    e.add_request("g", PROMPT, sp())
    e.add_request("t", PROMPT[3:], sp(temperature=0.8, seed=4))
    e.add_request("p", PROMPT[5:], sp(temperature=0.8, top_p=0.7, seed=4))
    e.add_request("k", PROMPT[7:], sp(top_k=3, min_p=0.5))   # greedy: no-op
    out = drain(e)
    assert all(len(v) == 10 for v in out.values())
    assert e._b_cs_plan is None


def test_top_p_plus_bias_takes_the_torch_path(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("sample_constrained called")
    e = fresh_engine()
    e.add_request("b", PROMPT, sp(temperature=0.9, top_p=0.9, seed=2))
    base = drain(e)["b"]
    banned = max(set(base), key=base.count)
    monkeypatch.setattr(ops, "sample_constrained", boom)
    e = fresh_engine()
    torch_rows = []
    real = e._sample_torch
    monkeypatch.setattr(e, "_sample_torch",
                        lambda lg, s: torch_rows.append(s.req_id) or real(lg, s))
    e.add_request("b", PROMPT, sp(temperature=0.9, top_p=0.9, seed=2, top_k=8,
                                  min_p=0.01,
                                  logit_bias=[[banned, -100.0]]))
    out = drain(e)["b"]
    assert banned not in out and len(out) == 10
    assert torch_rows == ["b"] * 10


def test_torch_path_top_k_one_is_argmax():
    e = fresh_engine()
    e.add_request("g", PROMPT, sp())
    base = drain(e)["g"]
    e = fresh_engine()
    e.add_request("k", PROMPT, sp(temperature=1.5, top_p=0.99, top_k=1,
                                  seed=9))
    assert drain(e)["k"] == base


def test_spec_eligibility():
    def spec_steps(**kw):
        e = fresh_engine(spec_lookup=4)
        e.add_request("s", [5, 6, 7, 8] * 8, sp(max_tokens=12, **kw))
        drain(e)
        return e.stats.get("spec_steps", 0)
    assert spec_steps() > 0
    assert spec_steps(top_k=5, min_p=0.1) > 0          # greedy: still eligible
    assert spec_steps(logit_bias=[[7, 1.0]]) == 0


def test_migration_carries_the_fields_token_exact():
    params = lambda: sp(**{**CONSTRAINED, "max_tokens": 14})   # noqa: E731
    ref_e = fresh_engine()
    ref_e.add_request("m", PROMPT, params())
    want = drain(ref_e)["m"]

    src, dst = fresh_engine(), fresh_engine()
    src.add_request("m", PROMPT, params())
    got = []
    for _ in range(6):
        got.extend(o.token_id for o in src.step())
    assert 0 < len(got) < 14
    src.request_extract("m")
    src.step()
    state = src.take_extracted("m")
    assert state["params"]["logit_bias"] == [[3, -100.0], [77, 2.5]]
    assert state["params"]["top_k"] == 6
    assert state["params"]["min_p"] == 0.02
    dst.queue_adopt(state)
    tail = drain(dst)["m"]
    assert dst.take_adopt_result("m") == "ok"
    assert got + tail == want
