"""The wide int4 GEMM (ops.w4a16_wide_linear / ops.w4a16_zp_wide_linear)
against the path that serves the same rows without it.

Kernel level.  Llama-3-8B projections (N, K) at M in ROWS, both weight
forms, four calls ALTERNATED in one process, in this order:
  (a)  the wide op with a caller-owned ``out`` and slab;
  (b1) the path _linear_w4 takes for (N, K, M) when the wide table is
       empty: the tiled op (``out`` and slab given) up to its row limit
       for the shape, else w4_dequant into one scratch + the bf16 GEMM;
  (c)  the model's bf16 GEMM on an unquantized weight;
  (b2) the same call as (b1), to show the spread of (b).
Every variant rotates over enough distinct weight buffers that its working
set exceeds the 256 MB last-level cache.  Device-event timing, warm-up,
median.  The bar: (a) <= min(b1, b2) + |b1 - b2|.

--sweep times (a) alone under forced ``splitk`` values.

End to end (--e2e).  Llama-3-8B ``quant="int4"``, one engine, the routing
table as committed and emptied (the routing before) alternated A B A B: waves of long prompts under chunked prefill (--chunk tokens a
step) while 16 other requests decode.  Prints the median wall time of the
mixed steps that carry all 16 + chunk rows.

Usage: python scripts/bench_w4a16_wide.py [--iters N] [--sweep]
                                          [--e2e [--chunk T]]
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
from resilient_llm_amd.ops import ref  # noqa: E402

SHAPES = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096),
          "down": (4096, 14336)}
ROWS = (160, 192, 224, 256, 320, 384, 512)
L3_BYTES = 256 << 20
DEV = "cuda"
Model = llama.LlamaForCausalLM


def timed(fn):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    fn()
    b.record()
    return a, b


def med(pairs):
    return statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3


def weights(N, K, zp, g):
    """Rotating (packed, scales or meta) buffers past the last-level cache."""
    G = K // 128
    n = L3_BYTES // (N * K // 2 + N * G * (4 if zp else 2)) + 2
    packed = [torch.randint(-2 ** 31, 2 ** 31 - 1, (N * K // 8,),
                            dtype=torch.int32, device=DEV, generator=g)
              for _ in range(n)]
    s = [0.003 * (1 + torch.rand(N, G, device=DEV, generator=g))
         for _ in range(n)]
    if zp:
        sm = [ref.w4_zp_meta(torch.randint(0, 16, (N, G), dtype=torch.uint8,
                                           device=DEV, generator=g), t.half())
              for t in s]
    else:
        sm = [t.bfloat16() for t in s]
    return packed, sm


def kernel_level(iters, zp):
    wide, tiled, dequant = (
        (ops.w4a16_zp_wide_linear, ops.w4a16_zp_tiled_linear,
         ops.w4_zp_dequant) if zp else
        (ops.w4a16_wide_linear, ops.w4a16_tiled_linear, ops.w4_dequant))
    form = "zp" if zp else "sym"
    print(f"{form:>4} {'shape':>8} {'M':>4} {'(a) wide':>9} {'(b1)':>8} "
          f"{'(b2)':>8} {'(c) bf16':>9} {'min(b)/a':>9} {'(b) is':>8} bar")
    rows = []
    for name, (N, K) in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(N + K)
        packed, sm = weights(N, K, zp, g)
        nq = len(packed)
        nw = L3_BYTES // (N * K * 2) + 2
        dense = [(0.02 * torch.randn(N, K, device=DEV, generator=g)).bfloat16()
                 for _ in range(nw)]
        scratch = torch.empty(N, K, dtype=torch.bfloat16, device=DEV)
        slab = torch.empty(max(ops.w4a16_wide_plan(N, K)[0] * 512,
                               ops.w4a16_tiled_plan(N, K)[0] * 256) * N,
                           dtype=torch.float32, device=DEV)
        tiled_rows = min(256, Model._W4_TILED_ROWS_BY_SHAPE.get((N, K), 256))
        for M in ROWS:
            x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)

            def a(i):
                wide(x, packed[i % nq], sm[i % nq], out=out, ws=slab)

            def b(i):
                if M <= tiled_rows:
                    tiled(x, packed[i % nq], sm[i % nq], out=out, ws=slab)
                else:
                    llama._linear(x, dequant(packed[i % nq], sm[i % nq],
                                             out=scratch))

            def c(i):
                llama._linear(x, dense[i % nw])

            for i in range(6):
                a(i), b(i), c(i)
            ts = [[], [], [], []]
            for i in range(iters):
                for t, fn in zip(ts, (a, b, c, b)):
                    t.append(timed(lambda: fn(i)))
            torch.cuda.synchronize()
            ta, tb1, tc, tb2 = map(med, ts)
            ok = ta <= min(tb1, tb2) + abs(tb1 - tb2)
            rows.append(dict(form=form, shape=name, M=M, wide_us=ta,
                             b1_us=tb1, b2_us=tb2, bf16_us=tc, passes=ok,
                             b="tiled" if M <= tiled_rows else "deq+gemm"))
            print(f"{form:>4} {name:>8} {M:4d} {ta:9.1f} {tb1:8.1f} "
                  f"{tb2:8.1f} {tc:9.1f} {min(tb1, tb2) / ta:9.2f} "
                  f"{rows[-1]['b']:>8} {'ok' if ok else 'FAILS'}", flush=True)
        del packed, sm, dense, scratch, slab
        torch.cuda.empty_cache()
    print(json.dumps({"w4a16_wide_kernel_level": rows}))


def sweep(iters):
    for name, (N, K) in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(N + K)
        packed, sm = weights(N, K, False, g)
        nq = len(packed)
        slab = torch.empty(8 * 512 * N, dtype=torch.float32, device=DEV)
        for M in (256, 512):
            x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            res = {}
            for sk in (1, 2, 3, 4, 6, 8):
                for i in range(4):
                    ops.w4a16_wide_linear(x, packed[i % nq], sm[i % nq], sk,
                                          out=out, ws=slab)
                ts = [timed(lambda: ops.w4a16_wide_linear(
                    x, packed[i % nq], sm[i % nq], sk, out=out, ws=slab))
                    for i in range(iters)]
                torch.cuda.synchronize()
                res[sk] = round(med(ts), 1)
            print(f"sweep {name} M={M} plan="
                  f"{ops.w4a16_wide_plan(N, K)[0]}: {res}", flush=True)
        del packed, sm, slab
        torch.cuda.empty_cache()


def e2e(rounds, chunk):
    from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
    cfg = llama.get_config("llama-3-8b")
    table = dict(Model._W4_WIDE_ROWS_BY_SHAPE)
    model = Model(cfg, device="cuda:0", dtype=torch.bfloat16, quant="int4")
    kv = PagedKVCache.for_model(cfg, 2048, device="cuda:0")
    eng = LLMEngine(model, kv, max_batch_size=64, max_queue=256,
                    max_prefill_tokens=chunk, chunk_size=chunk,
                    enable_prefix_caching=False)
    times = {"wide": [], "before": []}

    def wave(tag, sink):
        for i in range(16):
            eng.add_request(f"{tag}-d{i}", [5 + i, 9, 11],
                            SamplingParams(max_tokens=40))
        for _ in range(3):
            eng.step()
        for i in range(8):
            eng.add_request(f"{tag}-p{i}",
                            [(7 * i + 3 * t) % 1000 + 5 for t in range(1792)],
                            SamplingParams(max_tokens=2))
        rows_seen = []
        real = model._linear_w4

        def spy(x, name):
            rows_seen.append(x.shape[0])
            return real(x, name)
        model._linear_w4 = spy
        while eng.has_work():
            del rows_seen[:]
            torch.cuda.synchronize()
            t0 = time.monotonic()
            eng.step()
            torch.cuda.synchronize()
            if rows_seen and max(rows_seen) == 16 + chunk:
                sink.append((time.monotonic() - t0) * 1e3)
        model._linear_w4 = real

    for r in range(rounds + 1):                  # round 0 warms both up
        for tag in ("wide", "before"):
            Model._W4_WIDE_ROWS_BY_SHAPE = table if tag == "wide" else {}
            sink = []
            wave(f"{tag}{r}", sink)
            if r:
                times[tag].append(round(statistics.median(sink), 3))
            print(f"round {r} {tag}: {len(sink)} steps of {16 + chunk} rows, "
                  f"median {statistics.median(sink):.3f} ms", flush=True)
    Model._W4_WIDE_ROWS_BY_SHAPE = table
    print(json.dumps({"w4a16_wide_e2e_step_ms": times}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=448,
                    help="prompt tokens per mixed step, next to 16 decode rows")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ops.load_extension(required=True)
    if args.e2e:
        e2e(args.rounds, args.chunk)
    elif args.sweep:
        sweep(args.iters)
    else:
        kernel_level(args.iters, False)
        kernel_level(args.iters, True)


if __name__ == "__main__":
    main()
