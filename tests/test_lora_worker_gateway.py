"""LoRA adapters above the engine: the worker's ``adapters`` option, the
``adapter`` field over RPC (generate, generate_n, stream) and migration
blobs, several gateway aliases on one worker's base weights, failover,
and the config checks."""

import asyncio
import json
import os
import tempfile

import pytest
import torch

from resilient_llm_amd.config import ConfigError, load_config
from resilient_llm_amd.engine import SamplingParams
from resilient_llm_amd.gateway.app import GatewayApp
from resilient_llm_amd.gateway.http import Request
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.workers.base import (
    GenerationRequest, WorkerError, WorkerRegistry,
)
from resilient_llm_amd.workers.engine_worker import (
    EngineWorker, render_prompt,
)
from resilient_llm_amd.workers.rpc import RpcWorkerClient, WorkerRpcServer
from resilient_llm_amd.workers.stub import StubWorker

from lora_cases import random_adapter

MODEL = "tiny"
TEXT = "which adapter answers this?"


@pytest.fixture(scope="module")
def adapter_dirs():
    """Two PEFT directories, written by save_adapter."""
    root = tempfile.mkdtemp(prefix="rlli-lora-")
    model = LlamaForCausalLM(get_config(MODEL), device="cpu",
                             dtype=torch.float32, seed=11)
    model.add_adapter("x", *random_adapter(model, 4, seed=2, std=0.2))
    model.add_adapter("y", *random_adapter(model, 8, seed=3, std=0.2,
                                           targets=("q_proj", "v_proj")))
    return {n: model.save_adapter(n, os.path.join(root, n))
            for n in ("x", "y")}


def make_worker(adapters, label="w", **kw):
    kw.setdefault("num_blocks", 64)
    return EngineWorker(device="cpu", model_name=MODEL, device_label=label,
                        seed=11, adapters=adapters, **kw)


def greq(rid, adapter=None, text=TEXT, max_tokens=10, **kw):
    return GenerationRequest(request_id=rid, model=MODEL,
                             messages=[{"role": "user", "content": text}],
                             max_tokens=max_tokens, temperature=0.0,
                             adapter=adapter, **kw)


def engine_text(worker, adapter, max_tokens=10, text=TEXT):
    """The completion of a direct engine call (no worker API) under
    ``adapter`` on an engine of its own."""
    w = make_worker(None, label="direct")
    try:
        w.model.adapter_names = worker.model.adapter_names
        w.model.lora = worker.model.lora
        w.model.lora_scale = worker.model.lora_scale
        w.model.lora_slices = worker.model.lora_slices
        w._stop = True                      # drive the engine by hand
        w._work_event.set()
        w._thread.join(timeout=5)
        prompt = w.tokenizer.encode(render_prompt(
            [{"role": "user", "content": text}]))
        w.engine.add_request("d", prompt, SamplingParams(
            max_tokens=max_tokens, temperature=0.0), adapter=adapter)
        toks = []
        while w.engine.has_work():
            toks += [o.token_id for o in w.engine.step()]
        return w.tokenizer.decode(toks)
    finally:
        w._wd_wake.set()


# -------------------------------------------------------------- the worker
def test_worker_loads_adapters_and_serves_by_name(adapter_dirs):
    async def run():
        w = make_worker(adapter_dirs)
        try:
            assert (await w.health())["adapters"] == ["x", "y"]
            res = {a: await w.generate(greq(f"r-{a}", a))
                   for a in ("x", "y", None)}
            texts = {a: r.text for a, r in res.items()}
            assert len(set(texts.values())) == 3
            for a in ("x", "y", None):
                assert texts[a] == engine_text(w, a)
            grp = await w.generate_n([greq(f"g.c{i}", "y") for i in range(3)])
            assert [g.text for g in grp] == [texts["y"]] * 3
            assert w.engine.stats["forks"] == 2
            with pytest.raises(WorkerError, match="unknown adapter"):
                await w.generate(greq("bad", "nope"))
            with pytest.raises(WorkerError, match="unknown adapter"):
                await w.generate_n([greq(f"b.c{i}", "nope")
                                    for i in range(2)])
            assert not w._sinks and w.in_flight == 0
        finally:
            await w.close()
    asyncio.run(run())


def test_stub_worker_accepts_and_ignores_the_adapter():
    async def run():
        stub = StubWorker("0", {MODEL})
        a = await stub.generate(greq("s1", "x", max_tokens=4))
        b = await stub.generate(greq("s2", None, max_tokens=4))
        assert a.text == b.text and a.completion_tokens == 4
    asyncio.run(run())


def test_adapter_rides_rpc_generate_generate_n_and_stream(adapter_dirs):
    async def run():
        w = make_worker(adapter_dirs, max_batch_size=4)
        sock = os.path.join(tempfile.mkdtemp(prefix="rlli-lora-"), "w.sock")
        server = WorkerRpcServer(w, sock)
        await server.start()
        client = RpcWorkerClient("gpu:w", {MODEL}, sock)
        try:
            await client.connect(timeout=10)
            want = {a: (await w.generate(greq(f"w-{a}", a))).text
                    for a in ("x", "y", None)}
            assert len(set(want.values())) == 3
            for a in ("x", "y", None):
                got = await client.generate(greq(f"rpc-{a}", a))
                assert got.text == want[a]
                text = ""
                async for chunk in client.generate_stream(
                        greq(f"st-{a}", a, stream=True)):
                    text += chunk.text
                assert text == want[a]
            grp = await client.generate_n([greq(f"n.c{i}", "x")
                                           for i in range(2)])
            assert [g.text for g in grp] == [want["x"]] * 2
            with pytest.raises(WorkerError):
                await client.generate(greq("rpc-bad", "nope"))
            assert client.in_flight == 0
        finally:
            await client.close()
            await server.stop()
            await w.close()
    asyncio.run(run())


def test_migration_blob_carries_the_adapter(adapter_dirs):
    async def run():
        src = make_worker(adapter_dirs, "src")
        dst = make_worker(adapter_dirs, "dst")
        bare = make_worker(None, "bare")
        try:
            want = (await dst.generate(greq("ref", "x", max_tokens=40))).text

            async def start(rid):
                task = asyncio.ensure_future(
                    src.generate(greq(rid, "x", max_tokens=40)))
                for _ in range(500):
                    if any(len(s.output_ids) >= 3
                           for s in src.engine.running):
                        break
                    await asyncio.sleep(0.005)
                return task
            task = await start("mig")
            blob = await src.migrate_out("mig")
            await dst.migrate_in(blob)
            await src.release_migrated("mig")
            with pytest.raises(WorkerError):
                await task
            got = await dst.generate(greq("mig", "x", max_tokens=40))
            assert got.text == want and got.completion_tokens == 40
            # a worker without the adapter refuses the blob, typed
            task = await start("mig2")
            blob = await src.migrate_out("mig2")
            with pytest.raises(WorkerError, match="adoption failed"):
                await bare.migrate_in(blob)
            assert not bare.engine.has_work()
            await src.release_migrated("mig2")
            with pytest.raises(WorkerError):
                await task
        finally:
            for w in (src, dst, bare):
                await w.close()
    asyncio.run(run())


# ------------------------------------------------------------- the gateway
def lora_config(adapter_dirs, second_worker=False):
    def entry(alias, target, adapter, mid):
        lp = {"model": f"stub/{target}/{MODEL}", "adapters": adapter_dirs}
        if adapter:
            lp["adapter"] = adapter
        return {"model_name": alias, "litellm_params": lp,
                "model_info": {"id": mid}}
    data = {
        "cluster": {"port": 4999, "host": "127.0.0.1"},
        "model_list": [entry("tenant-x", "p", "x", "p/x"),
                       entry("tenant-y", "p", "y", "p/y"),
                       entry("base", "p", None, "p/base")],
        "router_settings": {"routing_strategy": "simple-shuffle"},
    }
    if second_worker:
        data["model_list"].append(entry("tenant-x-fb", "f", "x", "f/x"))
        data["router_settings"]["fallbacks"] = [
            {"tenant-x": ["tenant-x-fb"]}]
    return load_config(data=data)


async def post(app, alias, rid, max_tokens=10, **kw):
    body = {"model": alias, "max_tokens": max_tokens, "temperature": 0.0,
            "messages": [{"role": "user", "content": TEXT}]}
    body.update(kw)
    req = Request("POST", "/v1/chat/completions", {"x-request-id": rid},
                  json.dumps(body).encode(), "HTTP/1.1")
    resp = await app.handle(req)
    return resp.status, json.loads(resp.body), resp.headers


def test_two_aliases_share_one_worker_with_different_adapters(adapter_dirs):
    async def run():
        config = lora_config(adapter_dirs)
        assert config.worker_adapters("stub", "p") == adapter_dirs
        w = make_worker(config.worker_adapters("stub", "p"), "stub:p")
        registry = WorkerRegistry()
        registry.register("stub", "p", w)
        app = GatewayApp(config, registry)
        try:
            texts = {}
            for alias, adapter in (("tenant-x", "x"), ("tenant-y", "y"),
                                   ("base", None)):
                status, p, headers = await post(app, alias, f"rid-{alias}")
                assert status == 200, p
                assert headers["x-gateway-device"] == "stub:p"
                assert headers["x-gateway-model-id"] == \
                    f"p/{adapter or 'base'}"
                texts[adapter] = p["choices"][0]["message"]["content"]
                assert texts[adapter] == engine_text(w, adapter)
            assert len(set(texts.values())) == 3
            # n > 1 through the alias keeps its adapter too
            status, p, _ = await post(app, "tenant-y", "rid-n", n=2)
            assert status == 200
            assert [c["message"]["content"] for c in p["choices"]] == \
                [texts["y"]] * 2
            # one worker, one set of base weights, per-deployment buckets
            assert len(registry.all()) == 1
            assert len({id(s.limiter) for s in app.router.states}) == 3
            assert sorted(s.dep.model_id for s in app.router.states) == \
                ["p/base", "p/x", "p/y"]
        finally:
            await w.close()
    asyncio.run(run())


def test_failover_replay_keeps_the_adapter(adapter_dirs):
    async def run():
        config = lora_config(adapter_dirs, second_worker=True)
        first = make_worker(adapter_dirs, "stub:p")
        second = make_worker(adapter_dirs, "stub:f")
        registry = WorkerRegistry()
        registry.register("stub", "p", first)
        registry.register("stub", "f", second)
        app = GatewayApp(config, registry)
        try:
            _, clean, h = await post(app, "tenant-x", "rid-clean")
            assert h["x-gateway-device"] == "stub:p"
            _, base, _ = await post(app, "base", "rid-base")
            first.fault_mode = "error"
            status, p, headers = await post(app, "tenant-x", "rid-fo")
            assert status == 200
            assert headers["x-gateway-device"] == "stub:f"
            assert headers["x-gateway-fallback"] == "true"
            assert p["choices"][0]["message"] == \
                clean["choices"][0]["message"]
            assert p["choices"][0]["message"] != \
                base["choices"][0]["message"]
            first.fault_mode = "none"
        finally:
            await first.close()
            await second.close()
    asyncio.run(run())


# -------------------------------------------------------------- the config
def _cfg(model_list, pools=None):
    cluster = {"port": 4999}
    if pools:
        cluster["pools"] = pools
    return {"cluster": cluster, "model_list": model_list}


def test_config_rejects_an_adapter_the_worker_does_not_load():
    with pytest.raises(ConfigError, match="not in the adapters"):
        load_config(data=_cfg([
            {"model_name": "a", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "adapters": {"x": "/a/x"},
                "adapter": "z"}}]))
    # another worker's adapters do not count
    with pytest.raises(ConfigError, match="not in the adapters"):
        load_config(data=_cfg([
            {"model_name": "a", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "adapters": {"x": "/a/x"}}},
            {"model_name": "b", "litellm_params": {
                "model": "gpu/1/llama-3-8b", "adapter": "x"}}]))
    # a sibling alias on the same worker may declare them
    ok = load_config(data=_cfg([
        {"model_name": "a", "litellm_params": {
            "model": "gpu/0/llama-3-8b", "adapters": {"x": "/a/x"}}},
        {"model_name": "b", "litellm_params": {
            "model": "gpu/0/llama-3-8b", "adapter": "x"}}]))
    assert ok.worker_adapters("gpu", "0") == {"x": "/a/x"}
    assert ok.worker_adapters("gpu", "1") == {}
    with pytest.raises(ConfigError):
        load_config(data=_cfg([
            {"model_name": "a", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "adapters": ["x"]}}]))


def test_config_rejects_adapters_with_fp8_weights():
    with pytest.raises(ConfigError, match="quantization"):
        load_config(data=_cfg([
            {"model_name": "a", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "quantization": "fp8",
                "adapters": {"x": "/a/x"}, "adapter": "x"}}]))
    with pytest.raises(ConfigError, match="quantization"):
        load_config(data=_cfg([
            {"model_name": "a", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "quantization": "fp8"}},
            {"model_name": "b", "litellm_params": {
                "model": "gpu/0/llama-3-8b", "adapters": {"x": "/a/x"}}}]))


def test_config_rejects_adapters_on_a_tensor_parallel_pool():
    entry = {"model_name": "a", "litellm_params": {
        "model": "pool/big/llama-3-70b", "adapters": {"x": "/a/x"},
        "adapter": "x"}}
    with pytest.raises(ConfigError, match="tensor_parallel"):
        load_config(data=_cfg([entry], pools={
            "big": {"gpus": [0, 1, 2, 3], "tensor_parallel": 4}}))
    # a TP = 1 pool runs the same lockstep op stream: gpu/ workers only
    with pytest.raises(ConfigError, match="gpu/<device> workers only"):
        load_config(data=_cfg([entry], pools={
            "big": {"gpus": [0], "tensor_parallel": 1}}))
