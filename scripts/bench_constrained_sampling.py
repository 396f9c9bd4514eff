"""ops.sample_constrained (logit_bias + top_k + min_p on the device) vs
the per-row torch composition the engine would otherwise need, and what
constrained rows cost a graphed decode step.

(a) sample_constrained on R of [64, 128256] bf16 logits, R in {1, 8, 64},
    every row with top_k = 50, min_p = 0.05 and a 16-entry bias.  Device
    time via events, median after warm-up.
(b) the same result the way the engine's torch path computes it: a host
    loop over the rows (bias add, softmax, top-k / min-p mask, seeded
    multinomial) ending in ``.tolist()``.  That path synchronizes, so it
    is wall time around a drained device.
(c) Llama-3-8B engine, graphed decode at batch 64: ms/step for 64 plain
    temperature rows and for the same batch with 8 rows constrained; the
    ratio is the figure to look at.

Run it under a time limit of its own:
  timeout -k 10 900 python scripts/bench_constrained_sampling.py
"""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import resilient_llm_amd.ops as ops  # noqa: E402

B, V = 64, 128256
TOP_K, MIN_P, N_BIAS, TEMP = 50, 0.05, 16, 0.8


def bias_for(r):
    g = torch.Generator().manual_seed(100 + r)
    ids = sorted(torch.randperm(V, generator=g)[:N_BIAS].tolist())
    vals = (torch.rand(N_BIAS, generator=g) * 10 - 5).tolist()
    return [[i, v] for i, v in zip(ids, vals)]


def torch_composition(logits, rows, seeds, biases):
    """Per-row host loop modelled on LLMEngine._sample_torch."""
    toks = torch.zeros(len(rows), dtype=torch.int32, device=logits.device)
    for j, r in enumerate(rows):
        lg = logits[r].float().clone()
        ids = torch.tensor([i for i, _ in biases[j]], device=lg.device)
        lg[ids] += torch.tensor([v for _, v in biases[j]], device=lg.device)
        probs = torch.softmax(lg / TEMP, -1)
        floor = torch.maximum(MIN_P * probs.max(),
                              probs.topk(TOP_K).values[-1])
        probs = torch.where(probs >= floor, probs, torch.zeros_like(probs))
        probs = probs / probs.sum()
        gen = torch.Generator(device=lg.device)
        gen.manual_seed(seeds[r])
        toks[j] = torch.multinomial(probs, 1, generator=gen)[0]
    return toks.tolist()


def bench_op(iters):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16).cuda()
    temps = torch.full((B,), TEMP, dtype=torch.float32, device="cuda")
    seeds_l = list(range(1, B + 1))
    seeds = torch.tensor(seeds_l, dtype=torch.int64, device="cuda")
    for _ in range(20):
        ops.sample(logits, temps, seeds, 0)
    pairs = []
    for _ in range(iters):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        ops.sample(logits, temps, seeds, 0)
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    print(f"ops.sample gumbel B={B}: "
          f"{statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3:.1f}"
          f" us (for scale)")
    print(f"{'R':>3} {'(a) kernel us':>14} {'(b) torch us':>13} {'b/a':>7}")
    for R in (1, 8, 64):
        rows_l = list(range(R))
        biases = [bias_for(r) for r in rows_l]
        i32 = lambda x: torch.tensor(x, dtype=torch.int32,  # noqa: E731
                                     device="cuda")
        offs = [0]
        for b_ in biases:
            offs.append(offs[-1] + len(b_))
        args = (logits, i32(rows_l), temps, seeds, 0, i32([TOP_K] * R),
                torch.full((R,), MIN_P, device="cuda"), i32(offs),
                i32([i for b_ in biases for i, _ in b_]),
                torch.tensor([v for b_ in biases for _, v in b_],
                             device="cuda"))
        for _ in range(20):
            ops.sample_constrained(*args)
        pairs = []
        for _ in range(iters):
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            ops.sample_constrained(*args)
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        ku = statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3
        n_host = max(3, min(iters, 200 // R))
        torch_composition(logits, rows_l, seeds_l, biases)
        walls = []
        for _ in range(n_host):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_composition(logits, rows_l, seeds_l, biases)
            walls.append((time.perf_counter() - t0) * 1e6)
        tu = statistics.median(walls)
        print(f"{R:3d} {ku:14.1f} {tu:13.1f} {tu / ku:7.1f}")


def bench_engine(steps):
    from resilient_llm_amd.engine import (LLMEngine, PagedKVCache,
                                          SamplingParams)
    from resilient_llm_amd.engine.graph import install_graph_runner
    from resilient_llm_amd.models import LlamaForCausalLM, get_config
    cfg = get_config("llama-3-8b")
    model = LlamaForCausalLM(cfg, device="cuda:0", dtype=torch.bfloat16,
                             seed=0)
    kv = PagedKVCache.for_model(cfg, num_blocks=1024, device="cuda:0")
    engine = LLMEngine(model, kv, max_batch_size=B)
    install_graph_runner(engine)

    def run(n_constrained):
        for i in range(B):
            kw = {}
            if i < n_constrained:
                kw = dict(top_k=TOP_K, min_p=MIN_P, logit_bias=bias_for(i))
            engine.add_request(
                f"r{n_constrained}-{i}", list(range(5 + i, 133 + i)),
                SamplingParams(max_tokens=steps + 24, temperature=TEMP,
                               seed=1000 + i, stop_on_eos=False, **kw))
        while engine.waiting or engine.prefilling:
            engine.step()
        for _ in range(8):                  # settle into steady replays
            engine.step()
        assert len(engine.running) == B and not engine._b_torch_sampling
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            engine.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        assert len(engine.running) == B
        while engine.has_work():
            engine.step()
        return ms

    run(0)                                  # warm everything once
    plain = [run(0) for _ in range(2)]
    cons = [run(8) for _ in range(2)]
    p, c = min(plain), min(cons)
    print(f"(c) graphed decode, batch {B}, Llama-3-8B: "
          f"all plain {p:.3f} ms/step {plain}, 8 constrained "
          f"{c:.3f} ms/step {cons}, ratio {c / p:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ops.load_extension(required=True)
    bench_op(args.iters)
    if not args.no_engine:
        bench_engine(args.steps)


if __name__ == "__main__":
    main()
