"""Times of the Mixture-of-Experts ops at the qwen3-30b-a3b layer geometry
(hidden 2048, 128 experts of width 768, top 8, bf16).

Per T in {1, 4, 16, 64, 256, 2048}, alternated call by call so that clock
and cache drift hits all alike, each call timed with its own pair of device
events, the median of --runs calls after --warmup untimed rounds:

  route  ops.moe_route on the [T, 128] router logits
  hip    ops.moe_mlp (align, gate/up + SwiGLU, down, combine)
  loop   what it replaces: a Python loop over the experts some row chose,
         F.linear / ops.silu_mul / F.linear on the gathered rows and an
         index_add_ of the weighted result (the row lists are read back to
         the host, as that loop must)

Call i runs on weight set i % --layers with its own routing, so that a
small T does not find its experts in the 256 MB last-level cache from the
call before.  "bytes" is what the distinct chosen experts' weights weigh
(the streaming floor is bytes over the HBM rate); "hip_GBps" is bytes over
the hip time.  Prints one JSON line per T.

Usage: python scripts/bench_moe.py [--runs 50] [--warmup 5] [--layers 6]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from resilient_llm_amd import ops  # noqa: E402

DEV = "cuda:0"
H, I, E, K = 2048, 768, 128, 8


def alternate(fns, runs, warmup):
    """Median us per call of each fn(i), the fns alternated call by call."""
    for i in range(warmup):
        for fn in fns.values():
            fn(i)
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(True), torch.cuda.Event(True))
              for _ in range(runs)] for k in fns}
    for r in range(runs):
        for k, fn in fns.items():
            s, e = ev[k][r]
            s.record()
            fn(r)
            e.record()
    torch.cuda.synchronize()
    return {k: round(statistics.median(s.elapsed_time(e) * 1e3
                                       for s, e in v), 2)
            for k, v in ev.items()}


def expert_loop(x, ids, w, wgu, wd):
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in torch.unique(ids).tolist():
        tok, slot = (ids == e).nonzero(as_tuple=True)
        y = F.linear(ops.silu_mul(F.linear(x[tok], wgu[e])), wd[e])
        out.index_add_(0, tok, y.float() * w[tok, slot].unsqueeze(1))
    return out.to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--tokens", type=int, nargs="*",
                    default=[1, 4, 16, 64, 256, 2048])
    args = ap.parse_args()
    torch.manual_seed(0)
    L = args.layers
    wgu = [(torch.randn(E, 2 * I, H, device=DEV) * H ** -0.5).bfloat16()
           for _ in range(L)]
    wd = [(torch.randn(E, H, I, device=DEV) * I ** -0.5).bfloat16()
          for _ in range(L)]
    per_expert = (2 * I * H + H * I) * 2

    for T in args.tokens:
        x = torch.randn(T, H, device=DEV).bfloat16()
        logits = [torch.randn(T, E, device=DEV).bfloat16() for _ in range(L)]
        routed = [ops.moe_route(lg, K) for lg in logits]
        distinct = statistics.mean(
            int(torch.unique(ids).numel()) for ids, _ in routed)
        ref = expert_loop(x, *routed[0], wgu[0], wd[0]).float()
        got = ops.moe_mlp(x, *routed[0], wgu[0], wd[0]).float()
        diff = float((got - ref).abs().max() / ref.abs().max())

        us = alternate({
            "route": lambda i: ops.moe_route(logits[i % L], K),
            "hip": lambda i: ops.moe_mlp(x, *routed[i % L], wgu[i % L],
                                         wd[i % L]),
            "loop": lambda i: expert_loop(x, *routed[i % L], wgu[i % L],
                                          wd[i % L]),
        }, args.runs, args.warmup)
        nbytes = distinct * per_expert
        print(json.dumps({
            "tokens": T, "row_tile": 16 if T * K < 16 * E else 64,
            "distinct_experts": round(distinct, 1),
            "bytes": int(nbytes), "us": us,
            "hip_GBps": round(nbytes / us["hip"] / 1e3, 1),
            "max_diff_vs_loop_rel": round(diff, 5),
            "runs": args.runs}), flush=True)


if __name__ == "__main__":
    main()
