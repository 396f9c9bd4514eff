"""OpenAI logprobs through the worker and gateway layers: EngineWorker
over a CPU `tiny` engine, and the gateway over the stub worker (whose
entries are synthetic but well-formed)."""

import asyncio
import json

import pytest

from resilient_llm_amd.client import APIError
from resilient_llm_amd.workers.base import GenerationRequest
from resilient_llm_amd.workers.engine_worker import EngineWorker
from tests.gateway_harness import run_gateway

MSGS = [{"role": "user", "content": "What is resilient inference?"}]
ALIAS = "llama-cris-demo"


def greq(**kw):
    defaults = dict(request_id="lp1", model="tiny",
                    messages=[{"role": "user", "content": "hello world"}],
                    max_tokens=6)
    defaults.update(kw)
    return GenerationRequest(**defaults)


def check_entry(e, n_top):
    assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
    assert isinstance(e["token"], str)
    assert isinstance(e["logprob"], float) and -9999.0 <= e["logprob"] <= 0
    assert e["bytes"] == list(e["token"].encode("utf-8"))
    assert len(e["top_logprobs"]) == n_top
    prev = 0.0
    for t in e["top_logprobs"]:
        assert set(t) == {"token", "logprob", "bytes"}
        assert t["bytes"] == list(t["token"].encode("utf-8"))
        assert -9999.0 <= t["logprob"] <= prev
        prev = t["logprob"]
    json.dumps(e)                        # JSON-plain (no -inf, no tensors)


# ------------------------------------------------------------ worker
def test_engine_worker_generate_and_stream_entries():
    async def run():
        w = EngineWorker(device="cpu", model_name="tiny", device_label="gpu:t",
                         num_blocks=32)
        try:
            res = await w.generate(greq(logprobs=True, top_logprobs=3))
            assert res.completion_tokens == 6
            assert len(res.logprobs) == res.completion_tokens
            for e in res.logprobs:
                check_entry(e, 3)
                # greedy: the emitted token is the most likely one
                assert e["top_logprobs"][0]["logprob"] == e["logprob"]

            chunks = [c async for c in w.generate_stream(
                greq(request_id="lp2", logprobs=True, top_logprobs=2))]
            assert len(chunks) == 6
            for c in chunks:
                check_entry(c.logprob, 2)
                assert c.logprob["token"] == w.tokenizer.decode([c.token_id])
            # same prompt, greedy: the streamed numbers equal the final ones
            assert [c.logprob["logprob"] for c in chunks] == \
                [e["logprob"] for e in res.logprobs]

            # a stop sequence cuts the text, not the per-token list
            res2 = await w.generate(greq(request_id="lp3", logprobs=True,
                                         stop=[res.text[len(res.text) // 2:]]))
            assert len(res2.text) < len(res.text)
            assert len(res2.logprobs) == res2.completion_tokens == 6

            plain = await w.generate(greq(request_id="lp4"))
            assert plain.logprobs is None
            chunks = [c async for c in w.generate_stream(
                greq(request_id="lp5"))]
            assert all(c.logprob is None for c in chunks)
        finally:
            await w.close()
    asyncio.run(run())


def test_migrated_pre_tokens_keep_their_entries():
    """Adopted request: the tokens generated before migration replay with
    their saved records, so the re-attached client gets a complete list
    (final) and one entry per chunk (replayed stream)."""
    import dataclasses as dc
    from resilient_llm_amd.workers.base import WorkerMigrated

    async def run():
        req = GenerationRequest(
            request_id="lpm", model="tiny",
            messages=[{"role": "user", "content": "hello " * 30}],
            max_tokens=120, logprobs=True, top_logprobs=2)
        c = EngineWorker(device="cpu", model_name="tiny", num_blocks=64,
                         max_batch_size=4)
        want = await c.generate(dc.replace(req))
        for mode in ("final", "stream"):
            a = EngineWorker(device="cpu", model_name="tiny", num_blocks=64,
                             max_batch_size=4)
            b = EngineWorker(device="cpu", model_name="tiny", num_blocks=64,
                             max_batch_size=4)
            task = asyncio.create_task(a.generate(dc.replace(req)))
            while not (a.engine.running and a.engine.running[0].output_ids):
                await asyncio.sleep(0.002)
            blob = await a.migrate_out("lpm")
            await b.migrate_in(blob)
            await a.release_migrated("lpm")
            with pytest.raises(WorkerMigrated):
                await task
            if mode == "final":
                res = await b.generate(dc.replace(req))
                got = res.logprobs
                assert res.completion_tokens == want.completion_tokens
            else:
                got = [ch.logprob async for ch in
                       b.generate_stream(dc.replace(req))]
            assert len(got) == want.completion_tokens
            assert [e["token"] for e in got] == \
                [e["token"] for e in want.logprobs]
            for e, w_ in zip(got, want.logprobs):
                check_entry(e, 2)
                assert abs(e["logprob"] - w_["logprob"]) <= 1e-4
            await a.close()
            await b.close()
        await c.close()

    asyncio.new_event_loop().run_until_complete(run())


# ------------------------------------------------------------ gateway
def _post_raw(client, path, payload):
    return client._post(path, payload)


@pytest.mark.parametrize("extra", [
    {"logprobs": "yes"},
    {"logprobs": 1},
    {"logprobs": True, "top_logprobs": 21},
    {"logprobs": True, "top_logprobs": -1},
    {"logprobs": True, "top_logprobs": True},
    {"logprobs": True, "top_logprobs": 2.5},
    {"logprobs": True, "top_logprobs": "3"},
    {"top_logprobs": 3},
    {"logprobs": False, "top_logprobs": 3},
])
def test_chat_validation_400(extra):
    with run_gateway() as (client, *_):
        with pytest.raises(APIError) as ei:
            _post_raw(client, "/chat/completions",
                      {"model": ALIAS, "messages": MSGS, "max_tokens": 4,
                       **extra})
        assert ei.value.status == 400
        assert ei.value.body["error"]["type"] == "invalid_request_error"


@pytest.mark.parametrize("n", [6, -1, True, "2", 1.5])
def test_legacy_validation_400(n):
    with run_gateway() as (client, *_):
        with pytest.raises(APIError) as ei:
            _post_raw(client, "/completions",
                      {"model": ALIAS, "prompt": "hi", "max_tokens": 4,
                       "logprobs": n})
        assert ei.value.status == 400
        assert ei.value.body["error"]["type"] == "invalid_request_error"


def test_chat_non_stream_shape_and_untouched_default():
    with run_gateway() as (client, *_):
        plain = _post_raw(client, "/chat/completions",
                          {"model": ALIAS, "messages": MSGS, "max_tokens": 5})
        # key-for-key today's body: no logprobs key at all
        assert set(plain) == {"id", "object", "created", "model", "choices",
                              "usage"}
        assert set(plain["choices"][0]) == {"index", "message",
                                            "finish_reason"}
        off = _post_raw(client, "/chat/completions",
                        {"model": ALIAS, "messages": MSGS, "max_tokens": 5,
                         "logprobs": False})
        assert set(off["choices"][0]) == set(plain["choices"][0])

        r = _post_raw(client, "/chat/completions",
                      {"model": ALIAS, "messages": MSGS, "max_tokens": 5,
                       "logprobs": True, "top_logprobs": 4})
        assert set(r) == set(plain)
        assert set(r["choices"][0]) == {"index", "message", "finish_reason",
                                        "logprobs"}
        content = r["choices"][0]["logprobs"]["content"]
        assert len(content) == r["usage"]["completion_tokens"] == 5
        for e in content:
            check_entry(e, 4)
        assert "".join(e["token"] for e in content) == \
            r["choices"][0]["message"]["content"]

        r0 = _post_raw(client, "/chat/completions",
                       {"model": ALIAS, "messages": MSGS, "max_tokens": 3,
                        "logprobs": True})
        for e in r0["choices"][0]["logprobs"]["content"]:
            check_entry(e, 0)


def test_chat_stream_one_entry_per_token_chunk():
    with run_gateway() as (client, *_):
        events = list(client.chat.completions.create(
            model=ALIAS, messages=MSGS, max_tokens=6, stream=True,
            logprobs=True, top_logprobs=2,
            stream_options={"include_usage": True}))
        token_events = [e for e in events if e["choices"]]
        assert len(token_events) == 6
        for e in token_events:
            content = e["choices"][0]["logprobs"]["content"]
            assert len(content) == 1
            check_entry(content[0], 2)
            assert content[0]["token"] == e["choices"][0]["delta"]["content"]
        assert events[-1]["choices"] == [] and "usage" in events[-1]

        plain = list(client.chat.completions.create(
            model=ALIAS, messages=MSGS, max_tokens=4, stream=True))
        assert all("logprobs" not in e["choices"][0] for e in plain)


def test_stream_failover_each_entry_exactly_once():
    """A mid-stream worker fault re-routes and replays; the replay-skip
    drops the already-sent chunks WITH their entries."""
    with run_gateway(stub_kwargs={"token_delay_ms": 20}) as (client, registry,
                                                            _cfg):
        stream = client.chat.completions.create(
            model="llama-loadbalance-demo", messages=MSGS, max_tokens=12,
            stream=True, timeout=30, logprobs=True, top_logprobs=1)
        first = stream.headers["x-gateway-model-id"]
        tokens = []
        faulted = False
        for evt in stream:
            assert "error" not in evt, evt
            if not evt["choices"]:
                continue
            content = evt["choices"][0]["logprobs"]["content"]
            assert len(content) == 1
            tokens.append(content[0]["token"])
            if len(tokens) == 3 and not faulted:
                faulted = True
                client.inject_fault(
                    "stub:0" if "stub0" in first else "stub:1", "kill")
        assert faulted and any("failover" in c for c in stream.comments)
        client.inject_fault("stub:0", "none")
        client.inject_fault("stub:1", "none")
        from resilient_llm_amd.workers.stub import _CANNED
        want = [w if i == 0 else " " + w for i, w in enumerate(_CANNED[:12])]
        assert tokens == want


def test_legacy_completions_shape():
    with run_gateway() as (client, *_):
        none = _post_raw(client, "/completions",
                         {"model": ALIAS, "prompt": "hi", "max_tokens": 4})
        assert none["choices"][0]["logprobs"] is None

        r = _post_raw(client, "/completions",
                      {"model": ALIAS, "prompt": "hi", "max_tokens": 4,
                       "logprobs": 2})
        lp = r["choices"][0]["logprobs"]
        assert set(lp) == {"tokens", "token_logprobs", "top_logprobs",
                           "text_offset"}
        assert len(lp["tokens"]) == r["usage"]["completion_tokens"] == 4
        assert "".join(lp["tokens"]) == r["choices"][0]["text"]
        assert all(isinstance(v, float) and v <= 0
                   for v in lp["token_logprobs"])
        assert all(isinstance(d, dict) and len(d) == 2
                   and all(isinstance(v, float) for v in d.values())
                   for d in lp["top_logprobs"])
        offs, pos = [], 0
        for t in lp["tokens"]:
            offs.append(pos)
            pos += len(t)
        assert lp["text_offset"] == offs and offs[0] == 0

        r0 = _post_raw(client, "/completions",
                       {"model": ALIAS, "prompt": "hi", "max_tokens": 3,
                        "logprobs": 0})
        assert r0["choices"][0]["logprobs"]["top_logprobs"] == [{}, {}, {}]
        assert len(r0["choices"][0]["logprobs"]["token_logprobs"]) == 3


def test_client_round_trip():
    with run_gateway() as (client, *_):
        r = client.chat.completions.create(model=ALIAS, messages=MSGS,
                                           max_tokens=4, logprobs=True,
                                           top_logprobs=3)
        content = r.choices[0].logprobs.content
        assert len(content) == r.usage.completion_tokens == 4
        assert all(len(e.top_logprobs) == 3 and e.logprob <= 0
                   and e.top_logprobs[0].token == e.token for e in content)
        plain = client.chat.completions.create(model=ALIAS, messages=MSGS,
                                               max_tokens=4)
        assert plain.choices[0].get("logprobs") is None
