"""OpenAI ``n`` > 1 above the engine: Worker.generate_n (engine worker,
stub default, RPC, a TP=2 gloo pool) and the gateway (parsing, seeds,
one ticket / one charge / one ledger row, failover, legacy endpoint)."""

import asyncio
import hashlib
import json
import os
import tempfile
import time

import pytest

from resilient_llm_amd.config import PoolDef, load_config
from resilient_llm_amd.gateway.app import GatewayApp
from resilient_llm_amd.gateway.http import Request
from resilient_llm_amd.workers.base import (
    GenerationRequest, WorkerError, WorkerRegistry, WorkerThrottled,
)
from resilient_llm_amd.workers.engine_worker import EngineWorker
from resilient_llm_amd.workers.pool import spawn_pool_worker
from resilient_llm_amd.workers.rpc import RpcWorkerClient, WorkerRpcServer
from resilient_llm_amd.workers.stub import StubWorker

MODEL = "tiny-128"


def greq(rid, text="tell me a story about forks", max_tokens=10, seed=None,
         temperature=0.8, model=MODEL, **kw):
    return GenerationRequest(request_id=rid, model=model,
                             messages=[{"role": "user", "content": text}],
                             max_tokens=max_tokens, temperature=temperature,
                             seed=seed, **kw)


def make_worker(label="w", **kw):
    kw.setdefault("num_blocks", 64)
    return EngineWorker(device="cpu", model_name=MODEL, device_label=label,
                        seed=11, **kw)


async def settle(worker, timeout=10.0):
    """Wait until the engine has dropped everything it owned."""
    t0 = time.monotonic()
    eng = worker.engine
    while eng.has_work() or eng._live:
        assert time.monotonic() - t0 < timeout, "engine did not settle"
        await asyncio.sleep(0.01)
    assert eng.kv.free_blocks == eng.kv.num_blocks
    assert eng.n_active == 0 and not eng._attached


# ------------------------------------------------------------ engine worker
def test_generate_n_equals_three_generate_calls():
    async def run():
        w = make_worker()
        try:
            reqs = [greq(f"r.c{i}", seed=500 + i, logprobs=(i == 1),
                         top_logprobs=2 if i == 1 else 0) for i in range(3)]
            got = await w.generate_n(reqs)
            assert w.engine.stats["forks"] == 2
            assert not w._sinks and not w._group_rids and w.in_flight == 0
            want = [await w.generate(r) for r in reqs]
            assert w.engine.stats["forks"] == 2
            for g, x in zip(got, want):
                assert (g.text, g.prompt_tokens, g.completion_tokens,
                        g.finish_reason) == (x.text, x.prompt_tokens,
                                             x.completion_tokens,
                                             x.finish_reason)
                assert g.ttft_ms is not None and g.ttft_ms >= 0
            assert got[0].logprobs is None and got[2].logprobs is None
            assert [e["token"] for e in got[1].logprobs] == \
                [e["token"] for e in want[1].logprobs]
            assert all(len(e["top_logprobs"]) == 2 for e in got[1].logprobs)
            assert len({g.text for g in got}) > 1      # seeds differ
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_stop_sequence_cuts_one_choice_only():
    async def run():
        w = make_worker()
        try:
            base = [greq(f"s.c{i}", seed=40 + i, max_tokens=12)
                    for i in range(3)]
            plain = await w.generate_n(base)
            text1 = plain[1].text
            assert len(text1) > 2
            stop = text1[2:4]
            reqs = [greq(f"t.c{i}", seed=40 + i, max_tokens=12,
                         stop=[stop] if i == 1 else None) for i in range(3)]
            cut = await w.generate_n(reqs)
            assert cut[1].text == text1[:text1.find(stop)]
            assert cut[1].finish_reason == "stop"
            assert cut[1].completion_tokens == plain[1].completion_tokens
            for i in (0, 2):
                assert cut[i].text == plain[i].text
                assert cut[i].finish_reason == plain[i].finish_reason
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_failure_aborts_every_member_and_clears_sinks():
    async def run():
        w = make_worker()
        try:
            reqs = [greq(f"f.c{i}", seed=i, max_tokens=24) for i in range(4)]
            task = asyncio.ensure_future(w.generate_n(reqs))
            await asyncio.sleep(0)
            assert len(w._sinks) == 4 and w.in_flight == 4
            w.fault_mode = "error"
            with pytest.raises(WorkerError):
                await task
            assert not w._sinks and not w._group_rids and w.in_flight == 0
            w.fault_mode = "none"
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_group_over_capacity_is_throttled_and_leaves_nothing():
    async def run():
        w = make_worker(max_batch_size=2)
        try:
            with pytest.raises(WorkerThrottled):
                await w.generate_n([greq(f"x.c{i}", seed=i)
                                    for i in range(3)])
            assert not w._sinks and not w._group_rids and w.in_flight == 0
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_group_members_are_not_offered_for_migration():
    async def run():
        w = make_worker()
        try:
            reqs = [greq(f"m.c{i}", seed=i, max_tokens=24) for i in range(2)]
            task = asyncio.ensure_future(w.generate_n(reqs))
            solo = asyncio.ensure_future(
                w.generate(greq("solo", seed=9, max_tokens=24)))
            await asyncio.sleep(0)
            assert w.list_requests() == ["solo"]
            with pytest.raises(WorkerError, match="not live-migrated"):
                await w.migrate_out("m.c1")
            res = await task
            assert [r.completion_tokens > 0 for r in res] == [True, True]
            await solo
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_default_generate_n_on_the_stub():
    async def run():
        stub = StubWorker("0", {MODEL})
        res = await stub.generate_n([greq(f"q.c{i}", max_tokens=3 + i)
                                     for i in range(3)])
        assert [r.completion_tokens for r in res] == [3, 4, 5]
        stub.fault_mode = "error"
        with pytest.raises(WorkerError):
            await stub.generate_n([greq(f"e.c{i}") for i in range(3)])
        assert stub.in_flight == 0
    asyncio.run(run())


# ----------------------------------------------------------------------- RPC
def test_rpc_round_trip_of_generate_n():
    async def run():
        w = make_worker(max_batch_size=4)
        sock = os.path.join(tempfile.mkdtemp(prefix="rlli-n-"), "w.sock")
        server = WorkerRpcServer(w, sock)
        await server.start()
        client = RpcWorkerClient("gpu:w", {MODEL}, sock)
        try:
            await client.connect(timeout=10)
            reqs = [greq(f"rpc.c{i}", seed=70 + i, logprobs=True,
                         top_logprobs=1) for i in range(3)]
            got = await client.generate_n(reqs)
            want = await w.generate_n(reqs)
            assert [(g.text, g.completion_tokens, g.finish_reason)
                    for g in got] == \
                [(x.text, x.completion_tokens, x.finish_reason)
                 for x in want]
            assert [len(g.logprobs) for g in got] == \
                [g.completion_tokens for g in got]
            assert w.engine.stats["forks"] == 4
            assert client.in_flight == 0
            with pytest.raises(WorkerThrottled):
                await client.generate_n([greq(f"big.c{i}", seed=i)
                                         for i in range(5)])
            assert client.in_flight == 0 and not w._sinks
        finally:
            await client.close()
            await server.stop()
            await w.close()
    asyncio.run(run())


# ------------------------------------------------------------------ TP pool
@pytest.mark.timeout(240)
def test_tp2_generate_n_matches_tp1():
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    reqs = [greq(f"tp.c{i}", "fork the tensor parallel pool", 8,
                 seed=900 + i, model="tiny") for i in range(3)]

    async def reference():
        w = EngineWorker(device="cpu", model_name="tiny", device_label="ref",
                         num_blocks=64, seed=0)
        try:
            return await w.generate_n(reqs)
        finally:
            await w.close()
    want = asyncio.run(reference())

    sock = os.path.join(tempfile.mkdtemp(prefix="rlli-tpn-"), "pool.sock")
    pool = PoolDef(name="t", gpus=[0, 1], tensor_parallel=2)
    procs = spawn_pool_worker(pool, "tiny", sock, device_override="cpu",
                              tp_backend="gloo", max_batch=8)
    try:
        async def run():
            client = RpcWorkerClient("pool:t", {"tiny"}, sock)
            client.proc = procs[0]
            await client.connect(timeout=180)
            got = await client.generate_n(reqs)
            h = await client.health()
            await client.close()
            return got, h
        got, h = asyncio.run(run())
        assert [(g.text, g.completion_tokens) for g in got] == \
            [(x.text, x.completion_tokens) for x in want]
        assert h["engine_stats"]["forks"] == 2
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=10)
            except Exception:
                p.kill()


# ------------------------------------------------------------------ gateway
def gateway(workers: dict, fallbacks=True):
    """A GatewayApp over the given {target: worker}: alias 'gen' on the
    first, 'gen-fb' (its fallback) on the second."""
    targets = list(workers)
    model = MODEL
    data = {
        "cluster": {"port": 4999, "host": "127.0.0.1"},
        "model_list": [
            {"model_name": "gen",
             "litellm_params": {"model": f"stub/{targets[0]}/{model}"},
             "model_info": {"id": "primary"}}],
        "router_settings": {"routing_strategy": "simple-shuffle"},
    }
    if len(targets) > 1:
        data["model_list"].append(
            {"model_name": "gen-fb",
             "litellm_params": {"model": f"stub/{targets[1]}/{model}"},
             "model_info": {"id": "fallback"}})
        data["router_settings"]["fallbacks"] = [{"gen": ["gen-fb"]}]
    registry = WorkerRegistry()
    for t, w in workers.items():
        registry.register("stub", t, w)
    return GatewayApp(load_config(data=data), registry)


async def post(app, body, path="/v1/chat/completions", rid="rid-n-1"):
    req = Request("POST", path, {"x-request-id": rid},
                  json.dumps(body).encode(), "HTTP/1.1")
    resp = await app.handle(req)
    return resp.status, json.loads(resp.body), resp.headers


def chat_body(**kw):
    body = {"model": "gen", "max_tokens": 8, "temperature": 0.8, "seed": 77,
            "messages": [{"role": "user", "content": "fork this prompt"}]}
    body.update(kw)
    return body


def choice_seed(seed, i):
    return int.from_bytes(hashlib.blake2b(
        f"{seed}:{i}".encode(), digest_size=8).digest(), "big") >> 1


class Spy:
    """Count the router / consumer / ledger traffic of one app."""

    def __init__(self, app):
        self.acquired, self.completed, self.reconciled = [], [], []
        r_acq, r_done = app.router.acquire, app.router.complete
        c_rec = app.consumers.reconcile

        def acquire(alias, tokens_estimate=0, **kw):
            self.acquired.append(tokens_estimate)
            return r_acq(alias, tokens_estimate, **kw)

        def complete(ticket, actual_tokens=None):
            self.completed.append(actual_tokens)
            return r_done(ticket, actual_tokens=actual_tokens)

        def reconcile(key, estimated, actual):
            self.reconciled.append((estimated, actual))
            return c_rec(key, estimated, actual)

        app.router.acquire = acquire
        app.router.complete = complete
        app.consumers.reconcile = reconcile


def test_gateway_n3_over_the_engine_worker():
    async def run():
        w = make_worker("stub:p")
        app = gateway({"p": w})
        spy = Spy(app)
        try:
            status, one, _ = await post(app, chat_body())
            assert status == 200 and len(one["choices"]) == 1
            rows0 = len(app.ledger.recent(100))
            spy.acquired.clear(), spy.completed.clear()
            spy.reconciled.clear()

            status, p, headers = await post(app, chat_body(n=3, logprobs=True,
                                                           top_logprobs=2))
            assert status == 200
            assert [c["index"] for c in p["choices"]] == [0, 1, 2]
            assert p["id"] == "chatcmpl-rid-n-1"
            assert headers["x-request-id"] == "rid-n-1"
            # choice 0 is the n = 1 response for the same seed
            assert p["choices"][0]["message"] == one["choices"][0]["message"]
            assert p["choices"][0]["finish_reason"] == \
                one["choices"][0]["finish_reason"]
            # the others are what the documented derived seeds generate
            for i in (1, 2):
                lone = await w.generate(greq(
                    "lone", "fork this prompt", 8, seed=choice_seed(77, i)))
                assert p["choices"][i]["message"]["content"] == lone.text
                assert p["choices"][i]["finish_reason"] == lone.finish_reason
            per_choice = [len(c["logprobs"]["content"]) for c in p["choices"]]
            assert all(len(e["top_logprobs"]) == 2 for c in p["choices"]
                       for e in c["logprobs"]["content"])
            u = p["usage"]
            assert u["prompt_tokens"] == one["usage"]["prompt_tokens"]
            assert u["completion_tokens"] == sum(per_choice)
            assert u["total_tokens"] == u["prompt_tokens"] + sum(per_choice)
            # one ticket sized prompt + n * max_tokens, one charge of the
            # summed tokens, one ledger row
            prompt_est, _ = app._estimate(chat_body())
            assert spy.acquired == [prompt_est + 3 * 8]
            assert spy.completed == [u["total_tokens"]]
            assert spy.reconciled == [(prompt_est + 3 * 8, u["total_tokens"])]
            rows = app.ledger.recent(100)
            assert len(rows) == rows0 + 1
            assert rows[0]["request_id"] == "rid-n-1"
            assert rows[0]["status"] == "ok"
            assert rows[0]["prompt_tokens"] == u["prompt_tokens"]
            assert rows[0]["completion_tokens"] == u["completion_tokens"]
            assert w.engine.stats["forks"] == 2
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_gateway_greedy_n_yields_identical_choices():
    async def run():
        w = make_worker("stub:p")
        app = gateway({"p": w})
        try:
            body = chat_body(n=4, temperature=0.0)
            body.pop("seed")
            status, p, _ = await post(app, body)
            assert status == 200 and len(p["choices"]) == 4
            assert len({c["message"]["content"] for c in p["choices"]}) == 1
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_gateway_minted_seed_makes_n_replayable():
    """No client seed, temperature > 0: the seed minted from the request
    id drives every choice, so the same request id regenerates them all."""
    async def run():
        w = make_worker("stub:p")
        app = gateway({"p": w})
        try:
            body = chat_body(n=3)
            body.pop("seed")
            _, a, _ = await post(app, dict(body), rid="rid-mint")
            _, b, _ = await post(app, dict(body), rid="rid-mint")
            assert [c["message"] for c in a["choices"]] == \
                [c["message"] for c in b["choices"]]
            await settle(w)
        finally:
            await w.close()
    asyncio.run(run())


def test_gateway_n3_over_the_stub():
    async def run():
        app = gateway({"0": StubWorker("0", {MODEL})})
        spy = Spy(app)
        status, p, _ = await post(app, chat_body(n=3, max_tokens=5))
        assert status == 200
        assert [c["index"] for c in p["choices"]] == [0, 1, 2]
        assert all(c["finish_reason"] == "length" for c in p["choices"])
        assert all("logprobs" not in c for c in p["choices"])
        one_status, one, _ = await post(app, chat_body(max_tokens=5))
        assert p["choices"][0] == one["choices"][0]
        assert p["usage"]["prompt_tokens"] == one["usage"]["prompt_tokens"]
        assert p["usage"]["completion_tokens"] == 15
        assert spy.completed[0] == p["usage"]["total_tokens"]
        assert len(app.ledger.recent(100)) == 2
    asyncio.run(run())


@pytest.mark.parametrize("bad", [True, "2", 0, 17, 2.0, -1, [2]])
def test_gateway_bad_n_is_a_400(bad):
    async def run():
        app = gateway({"0": StubWorker("0", {MODEL})})
        status, p, _ = await post(app, chat_body(n=bad))
        assert status == 400 and "'n'" in p["error"]["message"]
        assert app.ledger.recent(10) == []
    asyncio.run(run())


def test_gateway_n_with_stream_is_a_400():
    async def run():
        app = gateway({"0": StubWorker("0", {MODEL})})
        status, p, _ = await post(app, chat_body(n=2, stream=True))
        assert status == 400
        assert "stream" in p["error"]["message"]
        # n = 1 may stream, 16 is the largest n
        resp = await app.handle(Request(
            "POST", "/v1/chat/completions", {},
            json.dumps(chat_body(n=1, stream=True)).encode(), "HTTP/1.1"))
        assert resp.status == 200 and resp.body_iter is not None
        await resp.body_iter.aclose()
        status, p, _ = await post(app, chat_body(n=16, max_tokens=2))
        assert status == 200 and len(p["choices"]) == 16
    asyncio.run(run())


def test_gateway_absent_n_is_unchanged():
    """Without 'n' (or with n = 1) the response is exactly the n = 1
    shape the gateway has always produced from one worker.generate."""
    async def run():
        stub = StubWorker("0", {MODEL})
        app = gateway({"0": stub})
        res = await stub.generate(greq("x", "fork this prompt", 8))
        status, p, headers = await post(app, chat_body(logprobs=True))
        status1, p1, headers1 = await post(app, chat_body(logprobs=True, n=1))
        assert status == status1 == 200
        created = p.pop("created")
        assert abs(created - time.time()) < 60
        p1.pop("created")
        assert p == p1 and headers == headers1
        assert p == {
            "id": "chatcmpl-rid-n-1",
            "object": "chat.completion",
            "model": "primary",
            "choices": [{
                "index": 0,
                "message": {"role": "assistant", "content": res.text},
                "finish_reason": res.finish_reason,
                "logprobs": {"content": (await stub.generate(greq(
                    "x", "fork this prompt", 8, logprobs=True))).logprobs},
            }],
            "usage": {
                "prompt_tokens": res.prompt_tokens,
                "completion_tokens": res.completion_tokens,
                "total_tokens": res.prompt_tokens + res.completion_tokens,
            },
        }
        assert headers == {
            "x-gateway-model-id": "primary", "x-gateway-device": "stub:0",
            "x-gateway-fallback": "false", "x-request-id": "rid-n-1",
            "content-type": "application/json"}
    asyncio.run(run())


def test_gateway_failover_takes_every_choice_from_the_second_worker():
    async def run():
        first = make_worker("stub:p")
        second = make_worker("stub:f")
        second.engine._arrival_counter = 1000   # default seeds cannot match
        app = gateway({"p": first, "f": second})
        try:
            _, clean, _ = await post(app, chat_body(n=3))
            first.fault_mode = "error"
            status, p, headers = await post(app, chat_body(n=3))
            assert status == 200
            assert headers["x-gateway-device"] == "stub:f"
            assert headers["x-gateway-fallback"] == "true"
            assert [c["message"] for c in p["choices"]] == \
                [c["message"] for c in clean["choices"]]
            assert second.engine.stats["forks"] == 2
            assert first.engine.stats["forks"] == 2      # the clean run only
            rows = app.ledger.recent(10)
            assert [r["status"] for r in rows] == ["ok", "error", "ok"]
            assert rows[0]["device"] == "stub:f"
            first.fault_mode = "none"
            await settle(first)
            await settle(second)
        finally:
            await first.close()
            await second.close()
    asyncio.run(run())


def test_legacy_completions_reshapes_every_choice():
    async def run():
        app = gateway({"0": StubWorker("0", {MODEL})})
        body = {"model": "gen", "prompt": "fork this prompt", "max_tokens": 4,
                "n": 2, "logprobs": 2}
        status, p, _ = await post(app, body, path="/v1/completions")
        assert status == 200 and p["object"] == "text_completion"
        assert [c["index"] for c in p["choices"]] == [0, 1]
        for c in p["choices"]:
            assert set(c) == {"index", "text", "logprobs", "finish_reason"}
            lp = c["logprobs"]
            assert len(lp["tokens"]) == len(lp["token_logprobs"]) == 4
            assert all(len(t) == 2 for t in lp["top_logprobs"])
            assert lp["text_offset"][0] == 0
            assert "".join(lp["tokens"]) == c["text"]
        assert p["usage"]["completion_tokens"] == 8
        status, p, _ = await post(app, dict(body, n=0), path="/v1/completions")
        assert status == 400
    asyncio.run(run())
