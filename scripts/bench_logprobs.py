"""ops.token_logprobs vs the torch composition the engine would otherwise
call (log_softmax(float) + topk + gather), with ops.sample for scale.

[64, 128256] bf16 logits (Llama-3 vocab at decode batch 64); R in
{1, 64} selected rows, k in {0, 5, 20}.  Device-event timing after
warm-up, one process, kernel and composition ALTERNATED call by call so
clock/neighbour drift hits both alike.  The kernel must read R*V*2
bytes; the printed GB/s is that over its time (the 16 MB input stays
cache-resident across iterations, so it is not an HBM rate).

Usage: python scripts/bench_logprobs.py [--iters N]
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
import resilient_llm_amd.ops as ops  # noqa: E402

B, V = 64, 128256


def torch_composition(logits, rows, tokens, k, full=False):
    """full: log_softmax over the whole [64, V] float copy, then pick the
    rows (the plain composition); else only the selected rows are
    widened — the cheapest torch can do."""
    if full:
        lp = torch.log_softmax(logits.float(), -1).index_select(
            0, rows.long())
    else:
        lp = torch.log_softmax(
            logits.index_select(0, rows.long()).float(), -1)
    chosen = lp.gather(1, tokens.long().unsqueeze(1)).squeeze(1)
    if k == 0:
        return chosen, None, None
    top_lp, top_ids = lp.topk(k, dim=-1)
    return chosen, top_lp, top_ids


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ops.load_extension(required=True)
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16).cuda()
    temps = torch.zeros(B, dtype=torch.float32, device="cuda")
    temps_s = torch.full((B,), 0.8, dtype=torch.float32, device="cuda")
    seeds = torch.arange(B, dtype=torch.int64, device="cuda")

    def med(pairs):
        return statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3

    for name, t in (("greedy", temps), ("gumbel", temps_s)):
        for _ in range(20):
            ops.sample(logits, t, seeds, 0)
        pairs = [timed(lambda: ops.sample(logits, t, seeds, 0))
                 for _ in range(args.iters)]
        torch.cuda.synchronize()
        print(f"ops.sample {name:6s} B={B}: {med(pairs):8.2f} us")

    print(f"{'R':>3} {'k':>3} {'kernel us':>10} {'torch us':>10} "
          f"{'speedup':>8} {'full us':>10} {'read GB/s':>10}")
    for R in (1, 64):
        rows = torch.arange(R, dtype=torch.int32, device="cuda")
        tokens = torch.randint(0, V, (R,), generator=g).to(torch.int32).cuda()
        for k in (0, 5, 20):
            for _ in range(20):
                ops.token_logprobs(logits, rows, tokens, k)
                torch_composition(logits, rows, tokens, k)
                torch_composition(logits, rows, tokens, k, full=True)
            kern, comp, full = [], [], []
            for _ in range(args.iters):
                kern.append(timed(
                    lambda: ops.token_logprobs(logits, rows, tokens, k)))
                comp.append(timed(
                    lambda: torch_composition(logits, rows, tokens, k)))
                full.append(timed(
                    lambda: torch_composition(logits, rows, tokens, k, True)))
            torch.cuda.synchronize()
            ku, cu, fu = med(kern), med(comp), med(full)
            print(f"{R:3d} {k:3d} {ku:10.2f} {cu:10.2f} {cu / ku:8.1f} "
                  f"{fu:10.2f} {R * V * 2 / ku / 1e3:10.1f}")


if __name__ == "__main__":
    main()
