"""Measurements behind profiles/shared_prefix_attn.md, on one GPU:

A. the op — ops.decode_attn_shared_qkv against ops.decode_attn_qkv on the
   same tensors at Llama-3-8B geometry (32 q heads, 8 kv heads, head_dim
   128): one group of 2 / 4 / 16 members sharing 1k / 8k / 32k tokens,
   64 private tokens each.  Device events, the two alternated over 5
   rounds of 40 calls after a warm-up; successive calls walk LAYERS
   different caches (>= 600 MB of K+V in all where 32 layers allow it) so
   that neither path is served from the last-level cache, as in a model
   whose weights stream between two visits of one layer.  Bytes are the
   K/V bytes each path has to read, from shapes.
B. end to end — one add_request_group of n = 16 on an 8k prompt, 64
   tokens, random-weight Llama-3-8B, shared_prefix_attention on against
   off, 3 alternated runs: host clock around the decode phase, which
   ends in a device synchronise, over its decode steps.

Usage: python scripts/bench_shared_prefix.py [--out result.json] [--skip-e2e]
"""

import argparse
import dataclasses
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
from resilient_llm_amd.engine.kv_cache import shared_prefix_groups  # noqa: E402
from resilient_llm_amd.models import LlamaForCausalLM, get_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the results here")
ap.add_argument("--skip-e2e", action="store_true")
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_shared_prefix needs a GPU"
DEV = "cuda:0"
res = {"device": torch.cuda.get_device_name(0), "op": []}


def flush():
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def time_it(fn, iters=40):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters       # us per call


# ------------------------------------------------------------------ A: op
N_Q, N_KV, D, BS, PRIVATE = 32, 8, 128, 16, 64
SCALE = D ** -0.5


def op_case(members, prefix):
    shared = prefix // BS
    own = -(-PRIVATE // BS)
    nb = shared + members * own
    per_layer = 2 * nb * N_KV * BS * D * 2
    layers = max(1, min(32, -(-600_000_000 // per_layer)))
    kc = torch.randn((layers, nb, N_KV, BS, D), device=DEV).to(torch.bfloat16)
    vc = torch.randn((layers, nb, N_KV, BS, D), device=DEV).to(torch.bfloat16)
    chains = [list(range(shared)) + list(range(shared + m * own,
                                               shared + (m + 1) * own))
              for m in range(members)]
    bt = torch.tensor(chains, dtype=torch.int32, device=DEV)
    lens = torch.full((members,), prefix + PRIVATE, dtype=torch.int32,
                      device=DEV)
    qkv = torch.randn((members, (N_Q + 2 * N_KV) * D),
                      device=DEV).to(torch.bfloat16)
    host = shared_prefix_groups(chains, [prefix + PRIVATE - 1] * members, BS,
                                BS, 64 // (N_Q // N_KV))
    chunks = ops.shared_prefix_chunks(len(host["tile_blocks"]), N_KV,
                                      -(-prefix // 64))
    T = len(host["tile_blocks"])
    plan = tuple(torch.tensor(host[k], dtype=torch.int32, device=DEV)
                 for k in ("n_shared", "row_tile", "row_slot", "tile_rows",
                           "tile_blocks", "tile_bt_row")) + (
        torch.empty((T, N_KV, chunks, 64, D), device=DEV),
        torch.empty((T, N_KV, chunks, 64, 2), device=DEV))

    def shared_fn(i):
        return ops.decode_attn_shared_qkv(qkv, kc[i % layers], vc[i % layers],
                                          bt, lens, plan, SCALE, N_Q)

    def base_fn(i):
        return ops.decode_attn_qkv(qkv, kc[i % layers], vc[i % layers], bt,
                                   lens, SCALE, N_Q)

    diff = (shared_fn(0).float() - base_fn(0).float()).abs().max().item()
    for fn in (shared_fn, base_fn):
        time_it(fn, 10)
    rounds = {"shared": [], "base": []}
    for _ in range(5):                                 # alternate the two
        rounds["shared"].append(time_it(shared_fn))
        rounds["base"].append(time_it(base_fn))
    kv_row = N_KV * D * 2 * 2                          # K+V bytes per token
    b_base = members * (prefix + PRIVATE) * kv_row
    b_shared = (prefix + members * PRIVATE) * kv_row
    med = {k: statistics.median(v) for k, v in rounds.items()}
    out = {"members": members, "prefix": prefix, "layers_rotated": layers,
           "chunks": chunks, "max_abs_diff": diff,
           "shared_us": med["shared"], "base_us": med["base"],
           "shared_us_range": [min(rounds["shared"]), max(rounds["shared"])],
           "base_us_range": [min(rounds["base"]), max(rounds["base"])],
           "base_over_shared": med["base"] / med["shared"],
           "shared_GBps": b_shared / med["shared"] / 1e3,
           "base_GBps": b_base / med["base"] / 1e3}
    print("op:", json.dumps(out), flush=True)
    return out


for prefix in (1024, 8192, 32768):
    for members in (2, 4, 16):
        res["op"].append(op_case(members, prefix))
        flush()
        torch.cuda.empty_cache()

if args.skip_e2e:
    sys.exit(0)

# ----------------------------------------------------------- B: end to end
cfg = dataclasses.replace(get_config("llama-3-8b"), max_position=16384)
model = LlamaForCausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=0)
kv = PagedKVCache.for_model(cfg, num_blocks=1024, device=DEV)
engines = {
    mode: LLMEngine(model, kv, max_batch_size=16, max_prefill_tokens=8192,
                    max_model_len=16384, enable_prefix_caching=False,
                    shared_prefix_attention=(mode == "on"))
    for mode in ("on", "off")}


def run(mode, rep):
    e = engines[mode]
    prompt = [(11 + 13 * rep + 7 * i) % 30000 + 5 for i in range(8192)]
    rids = [f"{mode}{rep}.c{i}" for i in range(16)]
    e.add_request_group(rids, prompt, [
        SamplingParams(max_tokens=64, temperature=0.8, seed=1000 + i,
                       stop_on_eos=False) for i in range(16)])
    while len(e.running) < 16:                         # prefill and fork
        e.step()
    torch.cuda.synchronize()
    steps0, t0 = e.stats["decode_steps"], time.monotonic()
    while e.has_work():
        e.step()
    torch.cuda.synchronize()
    return (time.monotonic() - t0) * 1e3 / (e.stats["decode_steps"] - steps0)


run("on", 100)                                         # warm both
run("off", 101)
ms = {"on": [], "off": []}
for rep in range(3):                                   # alternate the two
    ms["on"].append(run("on", 2 * rep))
    ms["off"].append(run("off", 2 * rep + 1))
res["e2e"] = {
    "model": "llama-3-8b (random weights)", "prompt_tokens": 8192,
    "max_tokens": 64, "n": 16, "ms_per_decode_step": ms,
    "on_median": statistics.median(ms["on"]),
    "off_median": statistics.median(ms["off"]),
    "shared_prefix_steps": engines["on"].stats["shared_prefix_steps"],
    "shared_prefix_rows": engines["on"].stats["shared_prefix_rows"]}
res["e2e"]["off_over_on"] = res["e2e"]["off_median"] / res["e2e"]["on_median"]
print("e2e:", json.dumps(res["e2e"]), flush=True)
flush()
