"""int4 weights (W4A16): the fused HIP GEMM against the alternatives, and
the 8B engine with and without ``quant="int4"``.

Kernel level.  Llama-3-8B projections (N, K) at M in {1, 16, 64}, three
variants ALTERNATED call by call in one process:
  (a) ops.w4a16_linear on the packed weight;
  (b) ops.w4_dequant into one scratch buffer + the bf16 GEMM the model
      calls (what rows > 64 take);
  (c) the model's bf16 GEMM on the unquantized weight.
Every variant rotates over enough distinct weight buffers that its
working set exceeds the 256 MB last-level cache: a decode step never
finds a weight in cache.  Device-event timing after warm-up, median.
Prints microseconds and packed bytes / time of (a).

End to end (--e2e).  The engine as the serving worker builds it (decode
graphs, batch 64), 64 requests of 128 prompt and 64 output tokens,
bf16 and int4 alternated A B A B.  Prints reqs/s and param_bytes().

Usage: python scripts/bench_w4a16.py [--iters N] [--e2e] [--model NAME]
"""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import resilient_llm_amd.ops as ops  # noqa: E402
from resilient_llm_amd.models import llama  # noqa: E402

SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]
ROWS = (1, 16, 64)
L3_BYTES = 256 << 20
DEV = "cuda"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def med(pairs):
    return statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3


def n_buffers(nbytes):
    return L3_BYTES // nbytes + 2


def kernel_level(iters, splitk):
    print(f"{'N':>6} {'K':>6} {'M':>3} {'(a) fused us':>13} "
          f"{'(b) deq+gemm us':>16} {'(c) bf16 us':>12} {'b/a':>6} {'c/a':>6} "
          f"{'(a) packed GB/s':>16}")
    rows = []
    for N, K in SHAPES:
        packed_bytes = N * K // 2 + N * K // 128 * 2
        nq, nw = n_buffers(packed_bytes), n_buffers(N * K * 2)
        g = torch.Generator(device=DEV).manual_seed(N + K)
        packed = [torch.randint(-2 ** 31, 2 ** 31 - 1, (N * K // 8,),
                                dtype=torch.int32, device=DEV, generator=g)
                  for _ in range(nq)]
        scales = [(0.003 * (1 + torch.rand(N, K // 128, device=DEV,
                                           generator=g))).bfloat16()
                  for _ in range(nq)]
        dense = [(0.02 * torch.randn(N, K, device=DEV, generator=g)).bfloat16()
                 for _ in range(nw)]
        scratch = torch.empty(N, K, dtype=torch.bfloat16, device=DEV)
        slab = torch.empty(ops.w4a16_plan(N, K, splitk)[0] * 64 * N,
                           dtype=torch.float32, device=DEV)
        for M in ROWS:
            x = torch.randn(M, K, device=DEV, generator=g).bfloat16()

            def fused(i):
                return ops.w4a16_linear(x, packed[i % nq], scales[i % nq],
                                        splitk, ws=slab)

            def deq_gemm(i):
                w = ops.w4_dequant(packed[i % nq], scales[i % nq],
                                   out=scratch)
                return llama._linear(x, w)

            def bf16(i):
                return llama._linear(x, dense[i % nw])

            for i in range(10):
                fused(i), deq_gemm(i), bf16(i)
            ta, tb, tc = [], [], []
            for i in range(iters):
                ta.append(timed(lambda: fused(i)))
                tb.append(timed(lambda: deq_gemm(i)))
                tc.append(timed(lambda: bf16(i)))
            torch.cuda.synchronize()
            a, b, c = med(ta), med(tb), med(tc)
            rows.append(dict(N=N, K=K, M=M, fused_us=a, deq_gemm_us=b,
                             bf16_us=c))
            print(f"{N:6d} {K:6d} {M:3d} {a:13.2f} {b:16.2f} {c:12.2f} "
                  f"{b / a:6.2f} {c / a:6.2f} {packed_bytes / a / 1e3:16.1f}",
                  flush=True)
        del packed, scales, dense, scratch, slab
        torch.cuda.empty_cache()
    lost = [r for r in rows if r["fused_us"] >= r["deq_gemm_us"]]
    print("gate (a) < (b) at every point:", "HOLDS" if not lost else
          f"FAILS at {[(r['N'], r['K'], r['M']) for r in lost]}")
    print(json.dumps({"w4a16_kernel_level": rows}))


def e2e(model_name, rounds):
    from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
    from resilient_llm_amd.engine.graph import install_graph_runner
    from resilient_llm_amd.models import LlamaForCausalLM, get_config
    cfg = get_config(model_name)
    engines = {}
    for quant in (None, "int4"):
        model = LlamaForCausalLM(cfg, device="cuda:0", dtype=torch.bfloat16,
                                 quant=quant)
        kv = PagedKVCache.for_model(cfg, 64 * 13 + 8, device="cuda:0")
        eng = LLMEngine(model, kv, max_batch_size=64, max_queue=256)
        install_graph_runner(eng)
        engines[quant or "bf16"] = eng
        print(f"{quant or 'bf16'}: param_bytes {model.param_bytes()} "
              f"({model.param_bytes() / 2 ** 30:.2f} GiB)", flush=True)

    def wave(eng, tag):
        for i in range(64):
            eng.add_request(f"{tag}-{i}",
                            [(7 * i + 3 * t) % 1000 + 5 for t in range(128)],
                            SamplingParams(max_tokens=64))
        torch.cuda.synchronize()
        t0 = time.monotonic()
        n = 0
        while eng.has_work():
            n += len(eng.step())
        torch.cuda.synchronize()
        dt = time.monotonic() - t0
        assert n == 64 * 64, n
        return 64 / dt

    res = {k: [] for k in engines}
    for r in range(rounds + 1):                  # round 0 warms both up
        for name, eng in engines.items():
            rate = wave(eng, f"{name}{r}")
            if r:
                res[name].append(rate)
            print(f"round {r} {name}: {rate:.1f} reqs/s"
                  + ("" if r else " (warm-up)"), flush=True)
    print(json.dumps({"w4a16_e2e_reqs_per_s": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--splitk", type=int, default=0)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ops.load_extension(required=True)
    if args.e2e:
        e2e(args.model, args.rounds)
    else:
        kernel_level(args.iters, args.splitk)


if __name__ == "__main__":
    main()
