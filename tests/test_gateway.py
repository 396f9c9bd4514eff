"""End-to-end gateway tests over HTTP with the CPU stub backend —
BASELINE.json config 1 (plumbing, no GPU)."""

import concurrent.futures as cf
import json
import time

import pytest

from resilient_llm_amd.client import APIError, RateLimitError
from tests.gateway_harness import run_gateway

MSGS = [{"role": "user", "content": "What is resilient inference?"}]


def test_basic_completion_and_headers():
    with run_gateway() as (client, registry, config):
        r = client.chat.completions.create(model="llama-cris-demo", messages=MSGS,
                                           max_tokens=8)
        assert r.choices[0].message.content
        assert r.usage.completion_tokens == 8
        assert r.model_id_header == "llama-cris-demo".replace("llama-cris-demo", r.model)
        assert r.device_header.startswith("stub:")
        assert r.object == "chat.completion"


def test_unknown_model_404():
    with run_gateway() as (client, *_):
        with pytest.raises(APIError) as ei:
            client.chat.completions.create(model="nope", messages=MSGS)
        assert ei.value.status == 404


def test_bad_body_400():
    with run_gateway() as (client, *_):
        with pytest.raises(APIError) as ei:
            client.chat.completions.create(model="llama-cris-demo", messages=[])
        assert ei.value.status == 400


def test_rate_limit_429_openai_body():
    """consumer-a rpm=3, no fallback: 4th+ request in the minute -> 429
    mapped to RateLimitError (X9, reference README.md:255-256)."""
    with run_gateway() as (client, *_):
        ok = 0
        limited = 0
        for _ in range(5):
            try:
                client.chat.completions.create(model="consumer-a-model",
                                               messages=MSGS, max_tokens=4)
                ok += 1
            except RateLimitError as e:
                assert e.body["error"]["type"] == "rate_limit_error"
                limited += 1
        assert ok == 3 and limited == 2


def test_fallback_transparent():
    """rpm=3 primary + fallback chain: 10 requests -> 3 primary, 7 on the
    fallback deployment, all successful (reference README.md:167-180)."""
    with run_gateway() as (client, *_):
        models = []
        for _ in range(10):
            r = client.chat.completions.create(model="llama-fallback-demo",
                                               messages=MSGS, max_tokens=4)
            models.append((r.model, r.was_fallback))
        primary = [m for m, fb in models if not fb]
        fallback = [m for m, fb in models if fb]
        assert len(primary) == 3 and len(fallback) == 7
        assert set(m for m, fb in models if fb) == {"stub1/llama-3-8b-fbq"}


def test_load_balancing_spreads():
    with run_gateway() as (client, *_):
        seen = set()
        for _ in range(6):
            r = client.chat.completions.create(model="llama-loadbalance-demo",
                                               messages=MSGS, max_tokens=4)
            seen.add(r.model_id_header)
        assert len(seen) >= 2   # 2 replicas + fallback pool once rpm spent


def test_concurrent_burst_cris_spread():
    """10 concurrent requests to the spread alias land on multiple stub
    devices and the distribution API reports them (X10/X12)."""
    with run_gateway() as (client, *_):
        def one(i):
            return client.chat.completions.create(
                model="llama-cris-demo", messages=MSGS, max_tokens=4).device_header
        with cf.ThreadPoolExecutor(10) as ex:
            devices = list(ex.map(one, range(10)))
        assert all(d.startswith("stub:") for d in devices)
        dist = client.distribution(by="device", alias="llama-cris-demo")
        assert dist["total"] == 10
        assert sum(dist["distribution"].values()) == 10
        assert set(dist["distribution"]) == set(devices)


def test_distribution_percentages_and_stats():
    with run_gateway() as (client, *_):
        for _ in range(4):
            client.chat.completions.create(model="llama-cris-demo",
                                           messages=MSGS, max_tokens=4)
        d = client.distribution(by="model_id")
        assert abs(sum(d["percentages"].values()) - 100.0) < 1.0
        st = d["stats"]
        assert st["ok"] == 4 and st["success_rate"] == 1.0
        assert st["latency_ms"]["p50"] is not None


def test_health_and_models_endpoints():
    with run_gateway() as (client, *_):
        h = client.health()
        assert h["status"] == "ok"
        assert all(w.get("status") == "ok" for w in h["workers"].values())
        models = client._get("/v1/models")
        ids = [m["id"] for m in models["data"]]
        assert "llama-fallback-demo" in ids


def test_router_admin_state():
    with run_gateway() as (client, *_):
        client.chat.completions.create(model="llama-fallback-demo",
                                       messages=MSGS, max_tokens=4)
        state = client.router_state()
        rows = {r["model_id"]: r for r in state["deployments"]}
        assert rows["stub0/llama-3-8b-primary"]["rpm_used"] == 1
        assert state["settings"]["routing_strategy"] == "simple-shuffle"


def test_fault_injection_reroutes():
    """Kill the primary worker: requests flow to the fallback deployment
    on the healthy device (X6 hot failover, no GPU needed)."""
    with run_gateway() as (client, registry, _):
        client.inject_fault("stub:0", "kill")
        r = client.chat.completions.create(model="llama-fallback-demo",
                                           messages=MSGS, max_tokens=4)
        assert r.was_fallback
        assert r.device_header == "stub:1"
        client.inject_fault("stub:0", "none")


def test_health_loop_marks_unhealthy_then_recovers():
    with run_gateway() as (client, registry, _):
        def healthy_becomes(want: bool) -> bool:
            # health loop interval 0.2s; poll instead of one fixed sleep
            # so a loaded machine only makes the test slower, not red
            deadline = time.monotonic() + 15.0
            while True:
                rows = {r["model_id"]: r
                        for r in client.router_state()["deployments"]}
                got = rows["stub0/llama-3-8b-primary"]["healthy"]
                if got is want or time.monotonic() > deadline:
                    return got is want
                time.sleep(0.05)

        client.inject_fault("stub:0", "kill")
        assert healthy_becomes(False)
        client.inject_fault("stub:0", "none")
        assert healthy_becomes(True)


def test_streaming_basic():
    with run_gateway() as (client, *_):
        stream = client.chat.completions.create(model="llama-cris-demo",
                                                messages=MSGS, max_tokens=6,
                                                stream=True)
        text, model = stream.collect_text()
        assert len(text.split()) == 6
        assert model


def test_streaming_midstream_failover():
    """Mid-stream worker death -> gateway replays on another deployment;
    client receives the full text exactly once (BASELINE config 4 shape)."""
    with run_gateway(stub_kwargs={"token_delay_ms": 20}) as (client, registry, _):
        stream = client.chat.completions.create(model="llama-loadbalance-demo",
                                                messages=MSGS, max_tokens=10,
                                                stream=True, timeout=30)
        first_device = stream.headers["x-gateway-model-id"]
        collected = []
        killed = False
        for evt in stream:
            for c in evt.get("choices", []):
                content = (c.get("delta") or {}).get("content")
                if content:
                    collected.append(content)
            if len(collected) == 3 and not killed:
                killed = True
                # kill whichever stub is serving
                dev = "stub:0" if "stub0" in first_device else "stub:1"
                client.inject_fault(dev, "kill")
        text = "".join(collected)
        assert len(text.split()) == 10, text
        assert killed
        client.inject_fault("stub:0", "none")
        client.inject_fault("stub:1", "none")


def test_metrics_endpoint():
    with run_gateway() as (client, *_):
        client.chat.completions.create(model="llama-cris-demo", messages=MSGS,
                                       max_tokens=2)
        conn = client._connect(None)
        conn.request("GET", "/metrics")
        body = conn.getresponse().read().decode()
        conn.close()
        assert "gateway_requests_total" in body
        assert "gateway_ledger_ok 1" in body
        # worker gauges appear once the health loop has swept
        import time as _t
        deadline = _t.time() + 5
        while _t.time() < deadline and "worker_in_flight" not in body:
            _t.sleep(0.3)
            conn = client._connect(None)
            conn.request("GET", "/metrics")
            body = conn.getresponse().read().decode()
            conn.close()
        assert "worker_in_flight" in body
        assert "worker_total_served" in body


def test_throttled_worker_typed_status():
    """Worker queue full -> typed Throttled (X13) -> retry on another
    deployment rather than hard failure."""
    with run_gateway(stub_kwargs={"max_concurrency": 1, "token_delay_ms": 30}) as \
            (client, registry, _):
        def one(i):
            try:
                r = client.chat.completions.create(model="llama-loadbalance-demo",
                                                   messages=MSGS, max_tokens=10,
                                                   timeout=30)
                return ("ok", r.device_header)
            except APIError as e:
                return ("err", e.status)
        with cf.ThreadPoolExecutor(4) as ex:
            results = list(ex.map(one, range(4)))
        oks = [r for r in results if r[0] == "ok"]
        assert len(oks) >= 2


def test_auth_policy_acl():
    """IAM-analogue ACL (C8): per-key alias allow-lists + admin gating."""
    from tests.gateway_harness import free_port, stub_config_dict
    port = free_port()
    cfg = stub_config_dict(port)
    cfg["auth"] = {
        "enforce": True,
        "keys": {
            "sk-a": {"allow": ["consumer-a-model"]},
            "sk-admin": {"allow": ["*"], "admin": True},
        },
        "default": {"allow": ["llama-cris-demo"], "admin": False},
    }
    with run_gateway(cfg) as (client, *_):
        from resilient_llm_amd.client import OpenAIClient
        base = f"http://127.0.0.1:{port}"
        a = OpenAIClient(base, api_key="sk-a")
        a.chat.completions.create(model="consumer-a-model", messages=MSGS,
                                  max_tokens=2)
        with pytest.raises(APIError) as ei:
            a.chat.completions.create(model="consumer-b-model", messages=MSGS)
        assert ei.value.status == 403
        # default key: open alias ok, admin denied
        anon = OpenAIClient(base, api_key="sk-unknown")
        anon.chat.completions.create(model="llama-cris-demo", messages=MSGS,
                                     max_tokens=2)
        with pytest.raises(APIError) as ei:
            anon.distribution()
        assert ei.value.status == 403
        admin = OpenAIClient(base, api_key="sk-admin")
        assert "distribution" in admin.distribution()
        # health stays open
        assert anon.health()["status"] == "ok"


def test_admin_requests_trace():
    with run_gateway() as (client, *_):
        client.chat.completions.create(model="llama-cris-demo", messages=MSGS,
                                       max_tokens=3)
        recs = client._get("/admin/requests", {"n": 10})["requests"]
        assert len(recs) == 1
        r = recs[0]
        assert r["alias"] == "llama-cris-demo" and r["status"] == "ok"
        assert r["completion_tokens"] == 3 and r["latency_ms"] > 0


def test_stream_client_disconnect_settles_ticket():
    """Dropping an SSE connection mid-stream must not leak router
    in-flight counts; the ledger records the cancellation."""
    with run_gateway(stub_kwargs={"token_delay_ms": 50}) as (client, registry, _):
        stream = client.chat.completions.create(
            model="llama-cris-demo", messages=MSGS, max_tokens=50,
            stream=True, timeout=30)
        it = iter(stream)
        next(it)
        stream._conn.close()   # hard client disconnect
        deadline = time.time() + 10
        settled = False
        while time.time() < deadline:
            rows = {r["model_id"]: r for r in client.router_state()["deployments"]}
            if all(r["in_flight"] == 0 for r in rows.values()):
                recs = client._get("/admin/requests", {"n": 20})["requests"]
                if any(r["status"] == "cancelled" for r in recs):
                    settled = True
                    break
            time.sleep(0.25)
        assert settled, "ticket not settled after client disconnect"


def test_consumer_limits_per_api_key():
    """Optional per-consumer buckets on top of per-deployment ones
    (SURVEY.md §3.4 MI355X equivalent)."""
    from tests.gateway_harness import free_port, stub_config_dict
    port = free_port()
    cfg = stub_config_dict(port)
    cfg["consumer_limits"] = {"keys": {"sk-limited": {"rpm": 2}}}
    with run_gateway(cfg) as (client, *_):
        from resilient_llm_amd.client import OpenAIClient
        limited = OpenAIClient(f"http://127.0.0.1:{port}", api_key="sk-limited")
        free = OpenAIClient(f"http://127.0.0.1:{port}", api_key="sk-free")
        ok = limited_429 = 0
        for _ in range(4):
            try:
                limited.chat.completions.create(model="llama-cris-demo",
                                                messages=MSGS, max_tokens=2)
                ok += 1
            except RateLimitError:
                limited_429 += 1
        assert ok == 2 and limited_429 == 2
        # other consumers unaffected
        for _ in range(4):
            free.chat.completions.create(model="llama-cris-demo",
                                         messages=MSGS, max_tokens=2)


def test_request_id_propagation():
    """x-request-id: client-supplied ids echo back and tag the ledger;
    absent ids are minted."""
    import http.client

    with run_gateway() as (client, registry, config):
        conn = http.client.HTTPConnection(client.host, client.port, timeout=15)
        body = json.dumps({"model": "llama-fallback-loadbalance",
                           "messages": [{"role": "user", "content": "id"}],
                           "max_tokens": 2})
        conn.request("POST", "/chat/completions", body=body,
                     headers={"content-type": "application/json",
                              "x-request-id": "req-my-trace-42"})
        resp = conn.getresponse()
        assert resp.status == 200
        assert resp.getheader("x-request-id") == "req-my-trace-42"
        resp.read()

        # minted when absent
        conn.request("POST", "/chat/completions", body=body,
                     headers={"content-type": "application/json"})
        resp2 = conn.getresponse()
        minted = resp2.getheader("x-request-id")
        assert minted and minted.startswith("req-") and minted != "req-my-trace-42"
        resp2.read()
        conn.close()

        import urllib.request
        with urllib.request.urlopen(
                f"http://{client.host}:{client.port}/admin/requests?n=10",
                timeout=10) as r:
            rows = json.loads(r.read())["requests"]
        assert "req-my-trace-42" in [row["request_id"] for row in rows]


def test_stream_include_usage():
    """stream_options.include_usage emits a final usage chunk with
    empty choices before [DONE] (OpenAI semantics)."""
    import http.client

    with run_gateway() as (client, registry, config):
        conn = http.client.HTTPConnection(client.host, client.port, timeout=15)
        body = json.dumps({"model": "llama-fallback-loadbalance",
                           "messages": [{"role": "user", "content": "u"}],
                           "max_tokens": 3, "stream": True,
                           "stream_options": {"include_usage": True}})
        conn.request("POST", "/chat/completions", body=body,
                     headers={"content-type": "application/json"})
        resp = conn.getresponse()
        raw = resp.read().decode()
        conn.close()
        datas = [json.loads(l[6:]) for l in raw.splitlines()
                 if l.startswith("data: ") and l != "data: [DONE]"]
        assert raw.rstrip().endswith("data: [DONE]")
        usage_chunks = [d for d in datas if d.get("usage")]
        assert len(usage_chunks) == 1
        assert usage_chunks[0]["choices"] == []
        assert usage_chunks[0]["usage"]["completion_tokens"] == 3
        # prompt_tokens is the worker's ACTUAL count (1-word prompt),
        # not the admission estimate that includes max_tokens
        assert usage_chunks[0]["usage"]["prompt_tokens"] < 10
        # content chunks don't carry usage
        assert all("usage" not in d for d in datas[:-1])


def test_max_completion_tokens_alias():
    """OpenAI's newer max_completion_tokens name is honored."""
    with run_gateway() as (client, registry, config):
        r = client.chat.completions.create(
            model="llama-fallback-loadbalance",
            messages=[{"role": "user", "content": "alias"}],
            max_tokens=128, max_completion_tokens=3)
        # explicit max_tokens wins when both present (it was set to the
        # client default of 128 here, so 128 is the cap, not 3)...
        assert r.usage.completion_tokens <= 128

        import http.client
        conn = http.client.HTTPConnection(client.host, client.port, timeout=15)
        body = json.dumps({"model": "llama-fallback-loadbalance",
                           "messages": [{"role": "user", "content": "x"}],
                           "max_completion_tokens": 3})
        conn.request("POST", "/chat/completions", body=body,
                     headers={"content-type": "application/json"})
        resp = json.loads(conn.getresponse().read())
        conn.close()
        assert resp["usage"]["completion_tokens"] == 3


def test_legacy_completions_endpoint():
    with run_gateway() as (client, registry, config):
        import http.client
        conn = http.client.HTTPConnection(client.host, client.port, timeout=15)
        body = json.dumps({"model": "llama-fallback-loadbalance",
                           "prompt": "complete me", "max_tokens": 3})
        conn.request("POST", "/v1/completions", body=body,
                     headers={"content-type": "application/json"})
        resp = conn.getresponse()
        assert resp.status == 200
        data = json.loads(resp.read())
        conn.close()
        assert data["object"] == "text_completion"
        assert data["id"].startswith("cmpl-")
        assert data["choices"][0]["text"]
        assert data["usage"]["completion_tokens"] == 3


def test_api_fuzz_never_5xx():
    """Deterministic mini-fuzz over the request surface: malformed and
    edge-case bodies must map to 2xx/4xx — never a 5xx (handler bugs)."""
    import http.client
    import random

    rng = random.Random(1234)
    bodies = [
        {},                                        # missing everything
        {"model": "nope"},                         # unknown alias, no messages
        {"model": "llama-fallback-loadbalance"},   # no messages
        {"model": "llama-fallback-loadbalance", "messages": []},
        {"model": "llama-fallback-loadbalance",
         "messages": [{"role": "user", "content": "x"}],
         "max_tokens": "three"},                   # bad type
        {"model": 5, "messages": [{"role": "user", "content": "x"}]},
        {"model": "llama-fallback-loadbalance",
         "messages": [{"role": "user", "content": "x"}],
         "temperature": -1.0, "top_p": 0.0},
        {"model": "llama-fallback-loadbalance",
         "messages": [{"role": "user", "content": "x"}],
         "stop": [""] * 10},
        {"model": "llama-fallback-loadbalance",
         "messages": [{"role": "user", "content": "x"}],
         "stop": 42},
        {"model": "llama-fallback-loadbalance",
         "messages": [{"role": "user", "content": "x"}],
         "presence_penalty": "NaNish"},
        {"model": "unknown-model",
         "messages": [{"role": "user", "content": "x"}]},
    ]
    # plus a few random-garbage structures
    for _ in range(8):
        bodies.append({"model": rng.choice(["llama-fallback-loadbalance", 7]),
                       "messages": rng.choice([None, "hi", [{"role": "user",
                                                            "content": "y"}]]),
                       rng.choice(["seed", "stream", "max_tokens"]):
                           rng.choice(["x", -5, 1.5, {}, []])})

    with run_gateway() as (client, registry, config):
        conn = http.client.HTTPConnection(client.host, client.port, timeout=15)
        for body in bodies:
            conn.request("POST", "/chat/completions", body=json.dumps(body),
                         headers={"content-type": "application/json"})
            resp = conn.getresponse()
            resp.read()
            assert resp.status < 500, (resp.status, body)
        # raw non-JSON body
        conn.request("POST", "/chat/completions", body=b"\x00\x01notjson",
                     headers={"content-type": "application/json"})
        resp = conn.getresponse()
        resp.read()
        conn.close()
        assert resp.status == 400
