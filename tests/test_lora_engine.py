"""Per-request LoRA adapters through the engine on the CPU reference path
(``tiny``, float32): equivalence with merged weights, batching, the
prefix cache, migration, n > 1 groups, logprobs, speculative decoding and
the PEFT round trip."""

import json
import os

import pytest
import torch

from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.engine.kv_cache import block_hash_chain
from resilient_llm_amd.models import LlamaForCausalLM, get_config

from lora_cases import merged_model, random_adapter

_CFG = get_config("tiny")


def make_model(adapters=True):
    model = LlamaForCausalLM(_CFG, device="cpu", dtype=torch.float32, seed=7)
    if adapters:
        model.add_adapter("zero", *random_adapter(model, 4, seed=1,
                                                  zero_b=True))
        model.add_adapter("x", *random_adapter(model, 4, seed=2, std=0.2))
        model.add_adapter("y", *random_adapter(
            model, 8, seed=3, std=0.2, targets=("q_proj", "v_proj")))
    return model


_MODEL = make_model()
_BASE = make_model(adapters=False)


def fresh_engine(model=None, **kw):
    kv = PagedKVCache.for_model(_CFG, 128, device="cpu")
    kv.k = kv.k.float()
    kv.v = kv.v.float()
    kw.setdefault("max_batch_size", 8)
    return LLMEngine(model or _MODEL, kv, **kw)


def drain(engine, max_steps=500):
    outs = {}
    for _ in range(max_steps):
        if not engine.has_work():
            break
        for o in engine.step():
            outs.setdefault(o.req_id, []).append(o)
    assert not engine.has_work()
    return outs


def tokens(outs):
    return {rid: [o.token_id for o in v] for rid, v in outs.items()}


def greedy(max_tokens=12, **kw):
    return SamplingParams(max_tokens=max_tokens, temperature=0.0,
                          stop_on_eos=False, **kw)


PROMPT = [5 + (7 * i) % 90 for i in range(37)]
PROMPT_B = [9 + (11 * i) % 80 for i in range(21)]


def alone(adapter, prompt=PROMPT, model=None, params=None, **kw):
    e = fresh_engine(model, **kw)
    e.add_request("r", prompt, params or greedy(), adapter=adapter)
    return tokens(drain(e))["r"]


def test_zero_b_adapter_equals_no_adapter():
    assert alone("zero") == alone(None)
    assert alone(None) == alone(None, model=_BASE)


def test_adapter_changes_greedy_tokens():
    base, x, y = alone(None), alone("x"), alone("y")
    assert x != base and y != base and x != y


def last_logits(model, prompt, adapter=None):
    kv = PagedKVCache.for_model(_CFG, 16, device="cpu")
    kv.k, kv.v = kv.k.float(), kv.v.float()
    n = len(prompt)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)      # noqa: E731
    kw = {}
    if adapter is not None:
        kw["adapter_idx"] = torch.full((n,), model.adapter_index(adapter),
                                       dtype=torch.int32)
    return model.forward_prefill(i32(prompt), i32(list(range(n))), kv,
                                 i32(list(range(n))), i32([0, n]), **kw)[0]


@pytest.mark.parametrize("name", ["x", "y"])
def test_unmerged_adapter_matches_merged_weights(name):
    """float32 model: running adapter ``name`` beside the base GEMMs equals
    a model whose weights were merged as W + scale * B @ A — the same
    greedy tokens, and last-position logits that differ only by f32
    reassociation (x @ (W + sBA)^T against x @ W^T + s (x @ A^T) @ B^T).

    Measured on the CPU: max |logit difference| 3.22e-6 (x) and 8.27e-7
    (y) on logits of magnitude ~1; the bound is 10x the larger one, since
    the reassociation error grows with depth, not with the adapter."""
    merged = merged_model(_MODEL, name, lambda: make_model(adapters=False))
    assert alone(name) == alone(None, model=merged)
    a = last_logits(_MODEL, PROMPT, name)
    b = last_logits(merged, PROMPT)
    diff = float((a - b).abs().max())
    print(f"adapter {name}: max |logit diff| = {diff:.3e}, "
          f"max |logit| = {float(b.abs().max()):.3f}")
    assert diff <= 3.22e-5
    # and the adapter is no rounding-level effect
    assert float((b - last_logits(_BASE, PROMPT)).abs().max()) > 1e-3


def test_mixed_batch_gives_each_request_its_alone_tokens():
    e = fresh_engine()
    e.add_request("x", PROMPT, greedy(), adapter="x")
    e.add_request("y", PROMPT_B, greedy(), adapter="y")
    e.add_request("n", PROMPT, greedy())
    got = tokens(drain(e))
    assert got["x"] == alone("x")
    assert got["y"] == alone("y", PROMPT_B)
    assert got["n"] == alone(None)
    assert e.kv.free_blocks == e.kv.num_blocks


def test_mixed_batch_through_chunked_prefill_and_decode_rows():
    """A late arrival prefills in chunks beside decoding adapter rows."""
    e = fresh_engine(chunk_size=16)
    e.add_request("x", PROMPT, greedy(), adapter="x")
    for _ in range(4):
        e.step()
    e.add_request("y", PROMPT_B, greedy(), adapter="y")
    e.add_request("n", PROMPT, greedy())
    got = {}
    for rid, v in tokens(drain(e)).items():
        got[rid] = v
    assert got["y"] == alone("y", PROMPT_B)
    assert got["n"] == alone(None)
    assert got["x"] == alone("x")[-len(got["x"]):]


def test_prefix_cache_is_salted_by_adapter():
    assert block_hash_chain(PROMPT, 16) == block_hash_chain(PROMPT, 16, b"")
    assert not set(block_hash_chain(PROMPT, 16)) & set(
        block_hash_chain(PROMPT, 16, b"adapter:x"))
    e = fresh_engine()
    n_full = (len(PROMPT) - 1) // e.block_size
    assert n_full == 2
    want = {a: alone(a) for a in ("x", "y", None)}
    for i, adapter in enumerate(("x", "y", None)):
        hits0 = e.kv.prefix_hits
        e.add_request(f"first{i}", PROMPT, greedy(), adapter=adapter)
        assert tokens(drain(e))[f"first{i}"] == want[adapter]
        assert e.kv.prefix_hits == hits0, adapter      # zero hits across them
    for i, adapter in enumerate(("x", "y", None)):
        hits0 = e.kv.prefix_hits
        e.add_request(f"again{i}", PROMPT, greedy(), adapter=adapter)
        assert tokens(drain(e))[f"again{i}"] == want[adapter]
        assert e.kv.prefix_hits == hits0 + n_full, adapter   # full hits


def test_unknown_adapter_raises_value_error():
    e = fresh_engine()
    with pytest.raises(ValueError, match="unknown adapter"):
        e.add_request("r", PROMPT, greedy(), adapter="nope")
    with pytest.raises(ValueError, match="unknown adapter"):
        e.add_request_group(["a", "b"], PROMPT, [greedy(), greedy()],
                            adapter="nope")
    with pytest.raises(ValueError, match="unknown adapter"):
        fresh_engine(_BASE).add_request("r", PROMPT, greedy(), adapter="x")
    assert not e.has_work() and e.n_active == 0


def test_extract_adopt_keeps_the_adapter_token_exact():
    want = alone("x", params=greedy(14))
    src, dst = fresh_engine(), fresh_engine()
    src.add_request("m", PROMPT, greedy(14), adapter="x")
    got = []
    for _ in range(6):
        got += [o.token_id for o in src.step()]
    assert 0 < len(got) < 14
    src.request_extract("m")
    src.step()
    state = src.take_extracted("m")
    assert state["adapter"] == "x" and state["kv"] is not None
    dst.queue_adopt(state)
    got += tokens(drain(dst))["m"]
    assert dst.take_adopt_result("m") == "ok"
    assert got == want
    assert want != alone(None, params=greedy(14))


def test_adopt_of_a_waiting_request_re_prefills_under_the_adapter():
    src, dst = fresh_engine(), fresh_engine()
    src.add_request("w", PROMPT, greedy(), adapter="y")
    src.request_extract("w")
    src.step()
    state = src.take_extracted("w")
    assert state["adapter"] == "y" and state["kv"] is None
    dst.queue_adopt(state)
    assert tokens(drain(dst))["w"] == alone("y")


def test_adopt_without_the_adapter_fails_typed():
    src = fresh_engine()
    dst = fresh_engine(_BASE)
    src.add_request("m", PROMPT, greedy(14), adapter="x")
    for _ in range(4):
        src.step()
    src.request_extract("m")
    src.step()
    state = src.take_extracted("m")
    dst.queue_adopt(state)
    dst.step()
    res = dst.take_adopt_result("m")
    assert isinstance(res, Exception) and "adapter 'x'" in str(res)
    # nothing runs on the base weights, nothing leaks
    assert not dst.has_work() and dst.n_active == 0
    assert dst.kv.free_blocks == dst.kv.num_blocks


def test_group_and_logprobs_under_an_adapter():
    lp = greedy(10, logprobs=True, top_logprobs=3)
    e = fresh_engine()
    rids = ["g.c0", "g.c1", "g.c2"]
    e.add_request_group(rids, PROMPT, [lp, greedy(10), greedy(10)],
                        adapter="x")
    outs = drain(e)
    assert e.stats["forks"] == 2
    single = fresh_engine()
    single.add_request("r", PROMPT, lp, adapter="x")
    want = drain(single)["r"]
    for rid in rids:
        assert [o.token_id for o in outs[rid]] == [o.token_id for o in want]
    for got_o, want_o in zip(outs["g.c0"], want):
        assert got_o.logprob == pytest.approx(want_o.logprob, abs=1e-5)
        assert [t for t, _ in got_o.top_logprobs] == \
            [t for t, _ in want_o.top_logprobs]
        assert got_o.top_logprobs[0][0] == got_o.token_id     # greedy
    assert all(o.logprob is None for o in outs["g.c1"])
    # the adapter's distribution, not the base model's
    base = fresh_engine()
    base.add_request("r", PROMPT, lp)
    assert [o.logprob for o in drain(base)["r"]] != [o.logprob for o in want]
    assert e.kv.free_blocks == e.kv.num_blocks


def test_spec_decode_equals_plain_decode_under_an_adapter():
    # a repetitive prompt, so prompt-lookup really proposes
    prompt = [7, 8, 9, 10, 11, 12] * 6
    p = greedy(24)
    plain = alone("x", prompt, params=p)
    e = fresh_engine(spec_lookup=4)
    e.add_request("s", prompt, p, adapter="x")
    e.add_request("n", prompt, p)
    got = tokens(drain(e))
    assert got["s"] == plain
    assert got["n"] == alone(None, prompt, params=p)
    assert e.stats.get("spec_steps", 0) > 0


def test_peft_directory_round_trip_is_bit_exact(tmp_path):
    model = make_model()
    dst = make_model(adapters=False)
    for name in ("x", "y"):                 # y targets q_proj + v_proj only
        path = model.save_adapter(name, str(tmp_path / name))
        assert sorted(os.listdir(path)) == ["adapter_config.json",
                                            "adapter_model.safetensors"]
        cfg = json.load(open(os.path.join(path, "adapter_config.json")))
        src = model._adapter_src[name]
        assert cfg["r"] == src["r"] and cfg["lora_alpha"] == src["lora_alpha"]
        assert cfg["target_modules"] == src["target_modules"]
        dst.load_adapter(name, path)
    assert dst.adapter_names == ["x", "y"]
    for name in ("x", "y"):
        a, b = model._adapter_src[name], dst._adapter_src[name]
        assert a["tensors"].keys() == b["tensors"].keys()
        for k in a["tensors"]:
            assert torch.equal(a["tensors"][k], b["tensors"][k])
    # stacked form: y (r = 8) pads x (r = 4); untargeted modules have zero B
    ix, iy = dst.adapter_index("x"), dst.adapter_index("y")
    A, B = dst.lora["l0.qkv"]
    assert A.shape == (2, 3 * 8, _CFG.hidden_size) and B.shape[2] == 8
    assert float(A[ix, 4:8].abs().max()) == 0.0       # rank padding
    assert float(B[ix, :, 4:].abs().max()) == 0.0
    q, kv = dst.q_size, dst.kv_size
    assert float(B[iy, q:q + kv].abs().max()) == 0.0   # k_proj not targeted
    assert float(B[iy, :q].abs().max()) > 0.0
    assert float(dst.lora["l1.o"][1][iy].abs().max()) == 0.0
    assert alone("y", model=dst) == alone("y")
    assert alone("x", model=dst) == alone("x")


def test_load_adapter_rejects_what_it_cannot_serve(tmp_path):
    model = make_model(adapters=False)
    r, alpha, targets, w = random_adapter(model, 4, seed=5)
    with pytest.raises(ValueError):
        model.add_adapter("big", 65, alpha, targets, w)
    with pytest.raises(ValueError):
        model.add_adapter("odd", r, alpha, ["embed_tokens"], w)
    with pytest.raises(KeyError):
        model.add_adapter("part", r, alpha, targets,
                          {k: v for k, v in list(w.items())[:-1]})
    assert model.adapter_names == [] and model.lora is None
    fp8 = LlamaForCausalLM(_CFG, device="cpu", dtype=torch.bfloat16, seed=7,
                           quant="fp8")
    with pytest.raises(RuntimeError):
        fp8.add_adapter("q", r, alpha, targets, w)
