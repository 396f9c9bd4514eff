"""Measurements behind profiles/kv_fork.md, on one GPU:

A. fork copy time — ops.kv_copy_blocks_ against the torch expression
   ``cache[:, dst] = cache[:, src]`` for K and V, Llama-3-8B cache shape,
   P = 3, device events, the two alternated over 7 rounds of 200 calls;
B. one n = 4 group (1024-token prompt, 64 tokens) against four concurrent
   n = 1 requests of the same prompt, with the KV blocks in use at the peak.

Usage: python scripts/bench_kv_fork.py [--out result.json]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from resilient_llm_amd import ops  # noqa: E402
from resilient_llm_amd.engine import (  # noqa: E402
    LLMEngine, PagedKVCache, SamplingParams)
from resilient_llm_amd.models import LlamaForCausalLM, get_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the results here")
OUT = ap.parse_args().out

assert torch.cuda.is_available(), "bench_kv_fork needs a GPU"
DEV = "cuda:0"
res = {"device": torch.cuda.get_device_name(0)}


def flush():
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)


# ------------------------------------------------------------ A: copy time
L, NB, H, BS, D = 32, 512, 8, 16, 128
k = torch.randn((L, NB, H, BS, D), device=DEV).to(torch.bfloat16)
v = torch.randn((L, NB, H, BS, D), device=DEV).to(torch.bfloat16)
src = torch.tensor([7, 7, 7], dtype=torch.int32, device=DEV)
dst = torch.tensor([10, 11, 12], dtype=torch.int32, device=DEV)
src_l, dst_l = src.long(), dst.long()
bytes_moved = 2 * 2 * L * 3 * H * BS * D * 2      # read + write, K and V


def run_kernel():
    ops.kv_copy_blocks_(k, v, src, dst)


def run_torch():
    k[:, dst_l] = k[:, src_l]
    v[:, dst_l] = v[:, src_l]


def time_it(fn, iters=200):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters       # us per call


for fn in (run_kernel, run_torch):
    for _ in range(20):
        fn()
torch.cuda.synchronize()
# correctness at the timed shape
kk, vv = k.clone(), v.clone()
run_kernel()
kk[:, dst_l] = kk[:, src_l]
vv[:, dst_l] = vv[:, src_l]
res["copy_matches_torch"] = bool(torch.equal(k.view(torch.int16),
                                             kk.view(torch.int16))
                                 and torch.equal(v.view(torch.int16),
                                                 vv.view(torch.int16)))
del kk, vv
rounds = {"kernel_us": [], "torch_us": []}
for _ in range(7):                                 # alternate the two
    rounds["kernel_us"].append(time_it(run_kernel))
    rounds["torch_us"].append(time_it(run_torch))
res["copy"] = {
    "shape": [L, NB, H, BS, D], "dtype": "bf16", "P": 3,
    "bytes_read_plus_written": bytes_moved,
    "kernel_us_median": statistics.median(rounds["kernel_us"]),
    "torch_us_median": statistics.median(rounds["torch_us"]),
    "kernel_us_rounds": rounds["kernel_us"],
    "torch_us_rounds": rounds["torch_us"],
}
res["copy"]["kernel_GBps"] = bytes_moved / res["copy"]["kernel_us_median"] / 1e3
print("copy:", json.dumps(res["copy"]), flush=True)
flush()
del k, v
torch.cuda.empty_cache()

# ----------------------------------------------------------- B: end to end
cfg = get_config("llama-3-8b")
model = LlamaForCausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
kv = PagedKVCache.for_model(cfg, num_blocks=1024, device=DEV)
engine = LLMEngine(model, kv, max_batch_size=8, max_prefill_tokens=8192)


def params(i):
    return SamplingParams(max_tokens=64, temperature=0.8, seed=1000 + i,
                          stop_on_eos=False)


def run(mode, rep):
    prompt = [(11 + 13 * rep + 7 * i) % 30000 + 5 for i in range(1024)]
    rids = [f"{mode}{rep}.c{i}" for i in range(4)]
    torch.cuda.synchronize()
    t0 = time.monotonic()
    if mode == "group":
        engine.add_request_group(rids, prompt, [params(i) for i in range(4)])
    else:
        for i, rid in enumerate(rids):
            engine.add_request(rid, prompt, params(i))
    peak = 0
    ttft = None
    n_tokens = 0
    while engine.has_work():
        outs = engine.step()
        if outs and ttft is None:
            torch.cuda.synchronize()
            ttft = time.monotonic() - t0
        n_tokens += len(outs)
        peak = max(peak, kv.num_blocks - kv.free_blocks)
    torch.cuda.synchronize()
    return {"total_ms": (time.monotonic() - t0) * 1e3,
            "first_tokens_ms": ttft * 1e3, "peak_blocks": peak,
            "tokens": n_tokens}


run("group", 100)                                  # warm both shapes
run("solo", 101)
e2e = {"group": [], "solo": []}
for rep in range(3):                               # alternate the two
    e2e["group"].append(run("group", 2 * rep))
    e2e["solo"].append(run("solo", 2 * rep + 1))
res["e2e"] = {
    "model": "llama-3-8b (random weights)", "prompt_tokens": 1024,
    "max_tokens": 64, "n": 4, "runs": e2e,
    "group_total_ms_median": statistics.median(
        r["total_ms"] for r in e2e["group"]),
    "solo_total_ms_median": statistics.median(
        r["total_ms"] for r in e2e["solo"]),
    "group_first_tokens_ms_median": statistics.median(
        r["first_tokens_ms"] for r in e2e["group"]),
    "solo_first_tokens_ms_median": statistics.median(
        r["first_tokens_ms"] for r in e2e["solo"]),
    "forks": engine.stats["forks"],
    "fork_shared_blocks": engine.stats["fork_shared_blocks"],
}
print("e2e:", json.dumps(res["e2e"]), flush=True)
flush()
