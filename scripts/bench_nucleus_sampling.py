"""ops.sample_nucleus (top_p and presence/frequency penalties on the
device) vs the per-row torch composition of LLMEngine._sample_torch, and
what such rows cost a graphed decode step with device_sampling on and off.

(a) sample_nucleus on R of [64, 128256] bf16 logits, R in {1, 8, 64}:
    top_p = 0.9 alone, and top_p + both penalties over a 256-token
    history.  Device time via events, median after warm-up.
(b) the same rows the way the engine's torch path serves them: a host
    loop (clone, count dict, softmax, sort + cumsum, multinomial from a
    fresh generator seeded with the row's plain seed) that reads each
    row's token back with ``int(...)``, as _sample_torch does.  Every row
    synchronizes, so it is wall time around a drained device.
(c) Llama-3-8B engine, graphed decode at batch 64 with 8 top_p rows:
    ms/step with device_sampling on and off.

Run it under a time limit of its own:
  timeout -k 10 900 python scripts/bench_nucleus_sampling.py
"""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import resilient_llm_amd.ops as ops  # noqa: E402

B, V = 64, 128256
TOP_P, PRES, FREQ, N_HIST, TEMP = 0.9, 0.5, 0.25, 256, 0.8


def history_for(r):
    g = torch.Generator().manual_seed(100 + r)
    return torch.randint(0, V, (N_HIST,), generator=g).tolist()


def torch_composition(logits, rows, seeds, hists):
    """Per-row host loop modelled on LLMEngine._sample_torch."""
    toks = []
    for j, r in enumerate(rows):
        lg = logits[r].float()
        if hists is not None:
            lg = lg.clone()
            counts = {}
            for t in hists[j]:
                counts[t] = counts.get(t, 0) + 1
            for t, c in counts.items():
                lg[t] -= PRES + FREQ * c
        probs = torch.softmax(lg / TEMP, -1)
        sp, idx = probs.sort(descending=True)
        keep = int((sp.cumsum(0) < TOP_P).sum()) + 1
        sp = sp[:keep] / sp[:keep].sum()
        gen = torch.Generator(device=lg.device)
        gen.manual_seed(seeds[r])
        toks.append(int(idx[int(torch.multinomial(sp, 1, generator=gen))]))
    return toks


def device_us(fn, iters):
    for _ in range(20):
        fn()
    pairs = []
    for _ in range(iters):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3


def bench_op(iters):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16).cuda()
    temps = torch.full((B,), TEMP, dtype=torch.float32, device="cuda")
    seeds_l = list(range(1, B + 1))
    seeds = torch.tensor(seeds_l, dtype=torch.int64, device="cuda")

    def i32(x):
        return torch.tensor(x, dtype=torch.int32, device="cuda")

    def f32(x):
        return torch.tensor(x, dtype=torch.float32, device="cuda")

    print(f"{'R':>3} {'rows':>10} {'(a) kernel us':>14} {'(b) torch us':>13}"
          f" {'b/a':>7}")
    for R in (1, 8, 64):
        rows_l = list(range(R))
        for name, pen in (("top_p", False), ("top_p+pen", True)):
            hists = [history_for(r) for r in rows_l] if pen else None
            history = i32(hists) if pen else i32([]).reshape(0, N_HIST)
            hist_len = i32([N_HIST] * R if pen else [])
            args = (logits, i32(rows_l), temps, seeds, 0, i32([0] * R),
                    f32([0.0] * R), f32([TOP_P] * R),
                    f32([PRES if pen else 0.0] * R),
                    f32([FREQ if pen else 0.0] * R), i32([0] * (R + 1)),
                    i32([]), f32([]), i32(rows_l if pen else [-1] * R),
                    history, hist_len, False)
            ku = device_us(lambda: ops.sample_nucleus(*args,
                                                      check_slots=False),
                           iters)
            torch_composition(logits, rows_l, seeds_l, hists)
            walls = []
            for _ in range(max(3, min(iters, 100 // R))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                torch_composition(logits, rows_l, seeds_l, hists)
                walls.append((time.perf_counter() - t0) * 1e6)
            tu = statistics.median(walls)
            print(f"{R:3d} {name:>10} {ku:14.1f} {tu:13.1f} {tu / ku:7.1f}")


def bench_engine(steps):
    from resilient_llm_amd.engine import (LLMEngine, PagedKVCache,
                                          SamplingParams)
    from resilient_llm_amd.engine.graph import install_graph_runner
    from resilient_llm_amd.models import LlamaForCausalLM, get_config
    cfg = get_config("llama-3-8b")
    model = LlamaForCausalLM(cfg, device="cuda:0", dtype=torch.bfloat16,
                             seed=0)

    def run(device_sampling, n_top_p):
        kv = PagedKVCache.for_model(cfg, num_blocks=1024, device="cuda:0")
        engine = LLMEngine(model, kv, max_batch_size=B,
                           device_sampling=device_sampling)
        install_graph_runner(engine)
        best = None
        for rep in range(3):                # the first one warms everything
            for i in range(B):
                kw = dict(top_p=TOP_P) if i < n_top_p else {}
                engine.add_request(
                    f"r{rep}-{i}", list(range(5 + i, 133 + i)),
                    SamplingParams(max_tokens=steps + 24, temperature=TEMP,
                                   seed=1000 + i, stop_on_eos=False, **kw))
            while engine.waiting or engine.prefilling:
                engine.step()
            for _ in range(8):              # settle into steady replays
                engine.step()
            assert len(engine.running) == B
            assert engine._b_torch_sampling == (n_top_p > 0
                                                and not device_sampling)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                engine.step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / steps
            while engine.has_work():
                engine.step()
            if rep:
                best = ms if best is None else min(best, ms)
        return best

    plain = run(False, 0)
    off = run(False, 8)
    on = run(True, 8)
    print(f"(c) graphed decode, batch {B}, Llama-3-8B, ms/step: all plain "
          f"{plain:.3f}; 8 top_p rows, device_sampling off {off:.3f}, "
          f"on {on:.3f}")


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
