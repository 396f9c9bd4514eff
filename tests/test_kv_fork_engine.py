"""n > 1 choices per request on the CPU engine (fp32, reference ops):
LLMEngine.add_request_group against the oracle that every member's
tokens equal those of a lone add_request with the same params on a fresh
engine — plus block accounting, aborts in every order, limits, the
per-member sampling features, the prefix cache and speculative decode."""

import dataclasses

import pytest
import torch

from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.engine.engine import CapacityExceeded
from resilient_llm_amd.models import LlamaForCausalLM, get_config

MODELS = ["tiny", "tiny-128"]
_MODEL_CACHE: dict = {}
_LONE_CACHE: dict = {}


def _model(name):
    if name not in _MODEL_CACHE:
        _MODEL_CACHE[name] = LlamaForCausalLM(
            get_config(name), device="cpu", dtype=torch.float32, seed=3)
    return _MODEL_CACHE[name]


def make_engine(name, num_blocks=64, **kw):
    kw.setdefault("enable_prefix_caching", False)
    kv = PagedKVCache.for_model(get_config(name), num_blocks, device="cpu",
                                kv_dtype=torch.float32)
    return LLMEngine(_model(name), kv, **kw)


def drain(engine, max_steps=1000):
    outs: dict = {}
    for _ in range(max_steps):
        if not engine.has_work():
            break
        for o in engine.step():
            outs.setdefault(o.req_id, []).append(o)
    assert not engine.has_work()
    return outs


def toks(outs):
    return {rid: [o.token_id for o in v] for rid, v in outs.items()}


def prompt_of(n):
    return [5 + (7 * i) % 90 for i in range(n)]


def sampled(i, max_tokens=12, **kw):
    return SamplingParams(max_tokens=max_tokens, temperature=0.8,
                          seed=100 + i, **kw)


def lone(name, prompt, params, **engine_kw):
    """The oracle: one add_request on a fresh engine (computed once per
    distinct case and shared)."""
    key = (name, tuple(prompt), repr(dataclasses.astuple(params)),
           repr(sorted(engine_kw.items())))
    if key not in _LONE_CACHE:
        e = make_engine(name, **engine_kw)
        e.add_request("lone", prompt, params)
        _LONE_CACHE[key] = drain(e)["lone"]
    return _LONE_CACHE[key]


def check_members(name, outs, prompt, members):
    for rid, p in members.items():
        want = lone(name, prompt, p)
        assert [o.token_id for o in outs[rid]] == \
            [o.token_id for o in want], rid
        assert outs[rid][-1].finish_reason == want[-1].finish_reason


# ------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("plen", [1, 16, 17, 37])
def test_group_members_equal_lone_runs(name, plen):
    prompt = prompt_of(plen)
    members = {f"g.c{i}": sampled(i) for i in range(4)}
    e = make_engine(name)
    e.add_request_group(list(members), prompt, list(members.values()))
    assert e.n_active == 4
    outs = drain(e)
    assert set(outs) == set(members)
    check_members(name, outs, prompt, members)
    assert e.stats["forks"] == 3
    assert e.stats["fork_shared_blocks"] == 3 * (plen // 16)
    assert e.kv.free_blocks == e.kv.num_blocks
    assert e.n_active == 0 and not e._live and not e._attached


@pytest.mark.parametrize("name", MODELS)
def test_group_of_one_is_a_plain_request(name):
    prompt = prompt_of(17)
    e = make_engine(name)
    e.add_request_group(["solo"], prompt, [sampled(0)])
    outs = drain(e)
    check_members(name, outs, prompt, {"solo": sampled(0)})
    assert e.stats["forks"] == 0
    assert e.kv.free_blocks == e.kv.num_blocks


@pytest.mark.parametrize("name", MODELS)
def test_fork_on_the_chunked_mixed_path(name):
    """chunk_size 16, 37-token prompt, an unrelated request already
    decoding: the fork happens on the mixed path after three chunks."""
    prompt = prompt_of(37)
    other_prompt = [9 + i for i in range(12)]
    other = SamplingParams(max_tokens=30, temperature=0.0)
    members = {f"g.c{i}": sampled(i) for i in range(4)}
    e = make_engine(name, chunk_size=16)
    e.add_request("other", other_prompt, other)
    first = e.step()
    assert [o.req_id for o in first] == ["other"]
    e.add_request_group(list(members), prompt, list(members.values()))
    outs = {"other": list(first)}
    steps_to_fork = 0
    while e.stats["forks"] == 0:
        for o in e.step():
            outs.setdefault(o.req_id, []).append(o)
        steps_to_fork += 1
    assert steps_to_fork == 3
    for rid, v in drain(e).items():
        outs.setdefault(rid, []).extend(v)
    check_members(name, outs, prompt, members)
    assert toks(outs)["other"] == [o.token_id for o in
                                   lone(name, other_prompt, other)]
    assert e.kv.free_blocks == e.kv.num_blocks


# ------------------------------------------------------- block accounting
@pytest.mark.parametrize("name", MODELS)
def test_block_accounting(name):
    prompt = prompt_of(37)
    members = {f"g.c{i}": sampled(i, max_tokens=8) for i in range(4)}
    e = make_engine(name, num_blocks=8)        # 4 lone requests need 12
    e.add_request_group(list(members), prompt, list(members.values()))
    e.step()
    assert e.stats["forks"] == 3
    # the leader's 3 blocks + one private block per child
    assert e.kv.num_blocks - e.kv.free_blocks == 6
    leader = next(s for s in e.running if s.req_id == "g.c0")
    for s in e.running:
        assert s.blocks[:2] == leader.blocks[:2]
        assert len(s.blocks) == 3
    assert len({s.blocks[2] for s in e.running}) == len(e.running)
    assert [s.req_id for s in e.running] == list(members)
    outs = {}
    for rid, v in drain(e).items():
        outs.setdefault(rid, []).extend(v)
    assert e.kv.free_blocks == e.kv.num_blocks
    assert sorted(e.kv._free) == list(range(8))


@pytest.mark.parametrize("name", MODELS)
def test_group_in_a_cache_of_8_blocks_completes(name):
    prompt = prompt_of(37)
    members = {f"g.c{i}": sampled(i, max_tokens=8) for i in range(4)}
    e = make_engine(name, num_blocks=8)
    e.add_request_group(list(members), prompt, list(members.values()))
    outs = drain(e)
    check_members(name, outs, prompt, members)
    # four independent requests do not fit at once
    e2 = make_engine(name, num_blocks=8)
    for rid, p in members.items():
        e2.add_request(rid, prompt, p)
    e2.step()
    assert len(e2.running) + len(e2.prefilling) == 2 and len(e2.waiting) == 2


def test_group_larger_than_the_cache_is_refused():
    e = make_engine("tiny", num_blocks=5)
    with pytest.raises(CapacityExceeded):
        e.add_request_group([f"c{i}" for i in range(4)], prompt_of(37),
                            [sampled(i, max_tokens=8) for i in range(4)])
    assert e.n_active == 0 and not e._live


# ------------------------------------------------------------------ aborts
def _group(e, n=4, plen=37, **kw):
    members = {f"g.c{i}": sampled(i) for i in range(n)}
    e.add_request_group(list(members), prompt_of(plen),
                        list(members.values()), **kw)
    return members


def _check_survivors(name, e, outs, members, gone):
    assert set(outs) == set(members) - set(gone)
    check_members(name, outs, prompt_of(37),
                  {r: p for r, p in members.items() if r not in gone})
    assert e.kv.free_blocks == e.kv.num_blocks
    assert not e._live and not e._attached and not e._aborted
    assert e.n_active == 0 and e._waiting_attached == 0


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("chunked", [False, True])
def test_abort_leader_before_fork(name, chunked):
    e = make_engine(name, chunk_size=16 if chunked else 2048)
    members = _group(e)
    if chunked:
        e.step()                       # leader admitted, mid-prefill
        assert e.prefilling and e.stats["forks"] == 0
    e.abort("g.c0")
    outs = drain(e)
    assert e.stats["forks"] == 3
    _check_survivors(name, e, outs, members, ["g.c0"])


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("chunked", [False, True])
def test_abort_one_child_before_fork(name, chunked):
    e = make_engine(name, chunk_size=16 if chunked else 2048)
    members = _group(e)
    if chunked:
        e.step()
    e.abort("g.c2")
    outs = drain(e)
    assert e.stats["forks"] == 2
    _check_survivors(name, e, outs, members, ["g.c2"])


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("chunked", [False, True])
def test_abort_every_member_before_fork(name, chunked):
    e = make_engine(name, chunk_size=16 if chunked else 2048)
    members = _group(e)
    if chunked:
        e.step()
        assert e.kv.free_blocks < e.kv.num_blocks
    for rid in members:
        e.abort(rid)
    outs = e.step()                    # dropped at the next step
    assert outs == [] and not e.has_work()
    assert e.stats["forks"] == 0
    _check_survivors(name, e, {}, members, list(members))


@pytest.mark.parametrize("name", MODELS)
def test_abort_leader_then_children_one_by_one(name):
    e = make_engine(name, chunk_size=16)
    members = _group(e)
    e.step()
    e.abort("g.c0")
    e.step()
    assert e.prefilling and e.prefilling[0].silent
    for rid in ("g.c1", "g.c2", "g.c3"):
        e.abort(rid)
    assert e.step() == [] and not e.has_work()
    _check_survivors(name, e, {}, members, list(members))


@pytest.mark.parametrize("name", MODELS)
def test_abort_child_after_fork(name):
    e = make_engine(name)
    members = _group(e)
    outs = {}
    for o in e.step():
        outs.setdefault(o.req_id, []).append(o)
    assert e.stats["forks"] == 3
    for o in e.step():
        outs.setdefault(o.req_id, []).append(o)
    e.abort("g.c1")
    for rid, v in drain(e).items():
        outs.setdefault(rid, []).extend(v)
    assert len(outs.pop("g.c1")) < 12
    _check_survivors(name, e, outs, members, ["g.c1"])


@pytest.mark.parametrize("name", MODELS)
def test_abort_leader_after_fork_keeps_shared_blocks(name):
    e = make_engine(name)
    members = _group(e)
    outs = {}
    for o in e.step():
        outs.setdefault(o.req_id, []).append(o)
    e.abort("g.c0")
    for rid, v in drain(e).items():
        outs.setdefault(rid, []).extend(v)
    outs.pop("g.c0")
    _check_survivors(name, e, outs, members, ["g.c0"])


def test_extract_before_fork_reports_missing_and_keeps_the_group():
    name = "tiny"
    e = make_engine(name, chunk_size=16)
    members = _group(e)
    e.step()
    e.request_extract("g.c0")
    e.request_extract("g.c2")
    e.step()
    assert e.take_extracted("g.c0") == "missing"
    assert e.take_extracted("g.c2") == "missing"
    outs = drain(e)
    _check_survivors(name, e, outs, members, [])


# ------------------------------------------------------------------ limits
def test_n_above_max_batch_size_raises():
    e = make_engine("tiny", max_batch_size=3)
    with pytest.raises(CapacityExceeded):
        _group(e, n=4)
    assert e.n_active == 0 and not e._live


def test_group_counts_n_against_max_queue():
    e = make_engine("tiny", max_queue=5)
    e.add_request("a", prompt_of(5), sampled(0))
    e.add_request("b", prompt_of(5), sampled(0))
    with pytest.raises(CapacityExceeded):
        _group(e, n=4)                 # 2 + 4 > 5
    _group(e, n=3)                     # 2 + 3 == 5
    assert e.n_active == 5
    with pytest.raises(CapacityExceeded):
        e.add_request("c", prompt_of(5), sampled(0))
    with pytest.raises(ValueError):
        e.add_request_group(["x", "x"], prompt_of(5), [sampled(0)] * 2)


def test_member_validation_matches_add_request():
    e = make_engine("tiny")
    bad = SamplingParams(max_tokens=4, top_logprobs=21)
    with pytest.raises(ValueError):
        e.add_request_group(["a", "b"], prompt_of(5), [sampled(0), bad])
    with pytest.raises(ValueError):
        e.add_request_group(["a", "b"], [10 ** 9], [sampled(0), sampled(1)])
    assert e.n_active == 0 and not e._live


@pytest.mark.parametrize("name", MODELS)
def test_group_waits_whole_for_batch_slots(name):
    prompt = prompt_of(37)
    other = SamplingParams(max_tokens=3, temperature=0.0)
    e = make_engine(name, max_batch_size=4)
    e.add_request("x", prompt_of(9), other)
    e.add_request("y", prompt_of(11), other)
    members = _group(e)                # needs 4 slots, 2 are taken
    e.step()
    assert [s.req_id for s in e.running] == ["x", "y"]
    assert [s.req_id for s in e.waiting] == ["g.c0"]
    assert e.stats["forks"] == 0 and e.n_active == 6
    outs = drain(e)
    assert outs["x"][-1].n_output_tokens == 3
    assert outs["y"][-1].n_output_tokens == 3
    _check_survivors(name, e, {r: outs[r] for r in members}, members, [])
    assert prompt == prompt_of(37)


# ---------------------------------------------------- per-member features
@pytest.mark.parametrize("name", MODELS)
def test_per_member_features(name):
    prompt = prompt_of(37)
    members = {
        "lp0": sampled(0, logprobs=True, top_logprobs=3),
        "plain": sampled(1),
        "lp2": SamplingParams(max_tokens=12, temperature=0.0, logprobs=True,
                              top_logprobs=3),
        "bias": sampled(3, logit_bias=[[40, 6.0], [7, -100.0]]),
        "topp": sampled(4, top_p=0.7),
        "topk": sampled(5, top_k=5, min_p=0.05),
    }
    e = make_engine(name)
    e.add_request_group(list(members), prompt, list(members.values()))
    outs = drain(e)
    check_members(name, outs, prompt, members)
    for rid, p in members.items():
        want = lone(name, prompt, p)
        for got, exp in zip(outs[rid], want):
            if p.logprobs:
                assert got.logprob == pytest.approx(exp.logprob, abs=1e-5)
                assert [t for t, _ in got.top_logprobs] == \
                    [t for t, _ in exp.top_logprobs]
                assert len(got.top_logprobs) == 3
            else:
                assert got.logprob is None and got.top_logprobs is None
    assert e.kv.free_blocks == e.kv.num_blocks


# ------------------------------------------------------------ prefix cache
@pytest.mark.parametrize("name", MODELS)
def test_second_group_reuses_cached_prefix(name):
    prompt = prompt_of(37)
    e = make_engine(name, enable_prefix_caching=True)
    first = {f"a.c{i}": sampled(i) for i in range(4)}
    e.add_request_group(list(first), prompt, list(first.values()))
    outs = drain(e)
    check_members(name, outs, prompt, first)
    assert e.kv.free_blocks == e.kv.num_blocks
    hits0 = e.kv.prefix_hits
    second = {f"b.c{i}": sampled(10 + i) for i in range(4)}
    e.add_request_group(list(second), prompt, list(second.values()))
    outs = drain(e)
    assert e.kv.prefix_hits == hits0 + 2       # the leader's two full blocks
    check_members(name, outs, prompt, second)
    assert e.stats["forks"] == 6
    assert e.kv.free_blocks == e.kv.num_blocks


# -------------------------------------------------------------- spec decode
@pytest.mark.parametrize("name", MODELS)
def test_spec_lookup_greedy_group(name):
    prompt = [11, 12, 13, 14, 15] * 7 + [11, 12]       # repetitive, 37
    greedy = SamplingParams(max_tokens=16, temperature=0.0)
    want = [o.token_id for o in lone(name, prompt, greedy)]
    e = make_engine(name, num_blocks=16, spec_lookup=4)
    rids = [f"s.c{i}" for i in range(4)]
    e.add_request_group(rids, prompt, [greedy] * 4)
    outs = {o.req_id: [o.token_id] for o in e.step()}
    # each member, leader included, holds the spec_lookup allowance
    assert all(len(s.blocks) == 4 + 1 for s in e.running)
    assert e.kv.num_blocks - e.kv.free_blocks == 5 + 3 * 3
    for rid, v in toks(drain(e)).items():
        outs[rid].extend(v)
    assert all(outs[r] == want for r in rids)
    assert e.stats.get("spec_steps", 0) > 0    # the forked batch speculated
    assert e.kv.free_blocks == e.kv.num_blocks
