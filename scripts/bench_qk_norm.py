"""Kernel times of the q/k-norm attention ops on the qwen3-8b attention
geometry (32 q heads, 8 kv heads, head_dim 128, bf16 cache, block 16).

Three alternatives per measurement point, alternated call by call so that
clock and cache state drift hits all of them alike; each call is timed
with its own pair of device events, the median of --runs calls is
reported after --warmup untimed rounds:

  new    ops.decode_attn_qknorm_rope_qkv / ops.qk_norm_rope_kv_append_qkv_
  (i)    the Llama op at the same shape (decode_attn_rope_qkv /
         rope_kv_append_qkv_): the cost of the norm
  (ii)   what the fusion replaces: ops.rmsnorm on the q and the k head
         views (strided views, so each is gathered, normalised and
         scattered back), then the Llama op

Decode: batch {1, 16, 64} x context {512, 4096}; unfused: {64, 512, 2048}
tokens.  Prints one JSON line per point.

Usage: python scripts/bench_qk_norm.py [--runs 200] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from resilient_llm_amd import ops  # noqa: E402

DEV = "cuda:0"
N_Q, N_KV, D, BS, EPS = 32, 8, 128, 16, 1e-6


def alternate(fns, runs, warmup):
    """Median us per call of each fn, the fns alternated call by call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(True), torch.cuda.Event(True))
              for _ in range(runs)] for k in fns}
    for r in range(runs):
        for k, fn in fns.items():
            s, e = ev[k][r]
            s.record()
            fn()
            e.record()
    torch.cuda.synchronize()
    return {k: round(statistics.median(s.elapsed_time(e) * 1e3
                                       for s, e in v), 2)
            for k, v in ev.items()}


def composed_norm(qkv, wq, wk):
    """ops.rmsnorm on the q and the k head views of qkv, in place."""
    T = qkv.shape[0]
    q = qkv[:, :N_Q * D]
    k = qkv[:, N_Q * D:(N_Q + N_KV) * D]
    q.copy_(ops.rmsnorm(q.reshape(T * N_Q, D), wq, EPS).view(T, N_Q * D))
    k.copy_(ops.rmsnorm(k.reshape(T * N_KV, D), wk, EPS).view(T, N_KV * D))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(0)
    wq = (1 + 0.25 * torch.randn(D)).to(torch.bfloat16).to(DEV)
    wk = (1 + 0.25 * torch.randn(D)).to(torch.bfloat16).to(DEV)
    W = (N_Q + 2 * N_KV) * D
    cs = ops.build_cos_sin(8192, D, 1e6, device=DEV)

    for B in (1, 16, 64):
        for L in (512, 4096):
            nb = (L + BS - 1) // BS
            kc = torch.randn(B * nb, N_KV, BS, D, device=DEV).to(torch.bfloat16)
            vc = torch.randn_like(kc)
            bt = torch.randperm(B * nb, device=DEV).view(B, nb).to(torch.int32)
            lens = torch.full((B,), L, dtype=torch.int32, device=DEV)
            pos = lens - 1
            slots = (bt[:, -1] * BS + (L - 1) % BS).to(torch.int32)
            src = torch.randn(B, W, device=DEV).to(torch.bfloat16)
            qkv = src.clone()
            scale = D ** -0.5

            def new():
                return ops.decode_attn_qknorm_rope_qkv(
                    src, wq, wk, EPS, pos, cs, kc, vc, slots, bt, lens,
                    scale, N_Q)

            def llama():
                return ops.decode_attn_rope_qkv(src, pos, cs, kc, vc, slots,
                                                bt, lens, scale, N_Q)

            def composed():
                composed_norm(qkv, wq, wk)
                return ops.decode_attn_rope_qkv(qkv, pos, cs, kc, vc, slots,
                                                bt, lens, scale, N_Q)

            us = alternate({"new": new, "llama_i": llama,
                            "composed_ii": composed}, args.runs, args.warmup)
            print(json.dumps({"op": "decode", "batch": B, "context": L,
                              "runs": args.runs, "us": us}), flush=True)

    for T in (64, 512, 2048):
        kc = torch.zeros((T + BS - 1) // BS, N_KV, BS, D, device=DEV,
                         dtype=torch.bfloat16)
        vc = torch.zeros_like(kc)
        pos = torch.arange(T, dtype=torch.int32, device=DEV)
        slots = pos.clone()
        # in-place ops: the values drift from call to call, the work does not
        a = torch.randn(T, W, device=DEV).to(torch.bfloat16)
        b, c = a.clone(), a.clone()

        def new():
            ops.qk_norm_rope_kv_append_qkv_(a, wq, wk, EPS, pos, cs, kc, vc,
                                            slots, N_Q)

        def llama():
            ops.rope_kv_append_qkv_(b, pos, cs, kc, vc, slots, N_Q)

        def composed():
            composed_norm(c, wq, wk)
            ops.rope_kv_append_qkv_(c, pos, cs, kc, vc, slots, N_Q)

        us = alternate({"new": new, "llama_i": llama,
                        "composed_ii": composed}, args.runs, args.warmup)
        print(json.dumps({"op": "unfused", "tokens": T, "runs": args.runs,
                          "us": us}), flush=True)


if __name__ == "__main__":
    main()
