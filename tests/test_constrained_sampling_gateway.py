"""logit_bias / top_k / min_p through the gateway (over the stub worker,
which accepts and ignores them), the legacy endpoint, the client and the
engine worker's vocab filter."""

import asyncio

import pytest

from resilient_llm_amd.client import APIError
from resilient_llm_amd.workers.base import GenerationRequest
from resilient_llm_amd.workers.stub import StubWorker
from tests.gateway_harness import run_gateway

MSGS = [{"role": "user", "content": "yes or no?"}]
ALIAS = "llama-cris-demo"


@pytest.fixture
def seen(monkeypatch):
    """GenerationRequests as the stub worker received them."""
    reqs = []
    real = StubWorker.generate

    async def recording(self, req):
        reqs.append(req)
        return await real(self, req)

    monkeypatch.setattr(StubWorker, "generate", recording)
    return reqs


@pytest.mark.parametrize("extra", [
    {"logit_bias": [[5, 1.0]]},
    {"logit_bias": "5"},
    {"logit_bias": {str(i): 1 for i in range(301)}},
    {"logit_bias": {"abc": 1}},
    {"logit_bias": {"-3": 1}},
    {"logit_bias": {"1.5": 1}},
    {"logit_bias": {"": 1}},
    {"logit_bias": {str(2 ** 31): 1}},
    {"logit_bias": {"7": 1, "07": 2}},
    {"logit_bias": {"7": "1"}},
    {"logit_bias": {"7": None}},
    {"logit_bias": {"7": True}},
    {"logit_bias": {"7": 100.5}},
    {"logit_bias": {"7": -101}},
    {"top_k": -1},
    {"top_k": 2.5},
    {"top_k": True},
    {"top_k": "4"},
    {"min_p": -0.01},
    {"min_p": 1.01},
    {"min_p": True},
    {"min_p": "0.1"},
])
def test_chat_validation_400(extra, seen):
    with run_gateway() as (client, *_):
        with pytest.raises(APIError) as ei:
            client._post("/chat/completions",
                         {"model": ALIAS, "messages": MSGS, "max_tokens": 4,
                          **extra})
        assert ei.value.status == 400
        assert ei.value.body["error"]["type"] == "invalid_request_error"
    assert seen == []


def test_valid_body_reaches_the_worker(seen):
    with run_gateway() as (client, *_):
        client._post("/chat/completions",
                     {"model": ALIAS, "messages": MSGS, "max_tokens": 4,
                      "logit_bias": {"900": -100, "7": 2.5, "31": 100},
                      "top_k": 40, "min_p": 0.05})
        client._post("/chat/completions",
                     {"model": ALIAS, "messages": MSGS, "max_tokens": 4,
                      "logit_bias": {}, "top_k": 0, "min_p": 0})
        client._post("/chat/completions",
                     {"model": ALIAS, "messages": MSGS, "max_tokens": 4})
    assert len(seen) == 3
    r = seen[0]
    assert r.logit_bias == [[7, 2.5], [31, 100.0], [900, -100.0]]
    assert all(type(i) is int and type(b) is float for i, b in r.logit_bias)
    assert r.top_k == 40 and r.min_p == 0.05
    defaults = GenerationRequest(request_id="", model="", messages=[])
    for r in seen[1:]:
        assert (r.logit_bias, r.top_k, r.min_p) == \
            (defaults.logit_bias, defaults.top_k, defaults.min_p) == \
            (None, 0, 0.0)


def test_legacy_completions_forwards(seen):
    with run_gateway() as (client, *_):
        client._post("/completions",
                     {"model": ALIAS, "prompt": "hi", "max_tokens": 4,
                      "logit_bias": {"12": -100}, "top_k": 3, "min_p": 0.5})
        with pytest.raises(APIError) as ei:
            client._post("/completions",
                         {"model": ALIAS, "prompt": "hi", "max_tokens": 4,
                          "top_k": -2})
        assert ei.value.status == 400
    assert len(seen) == 1
    assert seen[0].logit_bias == [[12, -100.0]]
    assert seen[0].top_k == 3 and seen[0].min_p == 0.5


def test_client_kwargs_only_when_given(monkeypatch):
    from resilient_llm_amd.client import OpenAIClient
    sent = []
    monkeypatch.setattr(OpenAIClient, "_post_json",
                        lambda self, path, payload, *a: sent.append(payload))
    c = OpenAIClient("http://127.0.0.1:1")
    c.chat.completions.create(model=ALIAS, messages=MSGS)
    c.chat.completions.create(model=ALIAS, messages=MSGS,
                              logit_bias={5: -100, 9: 1.5}, top_k=20,
                              min_p=0.1)
    assert not {"logit_bias", "top_k", "min_p"} & set(sent[0])
    assert sent[1]["logit_bias"] == {"5": -100, "9": 1.5}
    assert sent[1]["top_k"] == 20 and sent[1]["min_p"] == 0.1


def test_client_round_trip(seen):
    with run_gateway() as (client, *_):
        r = client.chat.completions.create(
            model=ALIAS, messages=MSGS, max_tokens=3,
            logit_bias={42: -100}, top_k=5, min_p=0.2)
        assert r.usage.completion_tokens == 3
    assert seen[0].logit_bias == [[42, -100.0]]
    assert seen[0].top_k == 5 and seen[0].min_p == 0.2


def test_engine_worker_passes_fields_and_drops_foreign_ids():
    from resilient_llm_amd.workers.engine_worker import EngineWorker

    async def run():
        w = EngineWorker(device="cpu", model_name="tiny", device_label="gpu:t",
                         num_blocks=32)
        try:
            vocab = w.engine.model.config.vocab_size
            req = dict(model="tiny", max_tokens=6,
                       messages=[{"role": "user", "content": "hello world"}])
            base = await w.generate(GenerationRequest(request_id="a", **req))
            captured = []
            real = w.engine.add_request
            w.engine.add_request = lambda rid, ids, params: (
                captured.append(params), real(rid, ids, params))[1]
            # an id past the vocab is dropped, not a worker failure
            forced = await w.generate(GenerationRequest(
                request_id="b", **req, top_k=7, min_p=0.25,
                logit_bias=[[65, 100.0], [vocab + 10, 5.0]]))
            assert forced.completion_tokens == 6
            assert forced.text == w.tokenizer.decode([65] * 6)
            assert forced.text != base.text
            p = captured[0]
            assert p.logit_bias == [[65, 100.0]]
            assert p.top_k == 7 and p.min_p == 0.25
            only_foreign = await w.generate(GenerationRequest(
                request_id="c", **req, logit_bias=[[vocab, 50.0]]))
            assert only_foreign.text == base.text
            assert captured[1].logit_bias is None
        finally:
            await w.close()
    asyncio.run(run())
