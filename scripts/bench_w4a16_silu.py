"""SwiGLU fused into the int4 down projection: where it pays.

Kernel level.  The Llama-3-8B down projection (N = 4096, K = 14336) at
M in {1, 8, 16, 32, 64}, two variants ALTERNATED call by call:
  (f) ops.w4a16_silu_linear on gu [M, 2K];
  (p) ops.silu_mul + ops.w4a16_linear, the pair it replaces;
and the same for the zero-point ops (--zp).  Both rotate over enough
packed weights that the working set exceeds the 256 MB last-level cache,
and over as many gu buffers.  Device-event timing after warm-up, median.

Usage: python scripts/bench_w4a16_silu.py [--iters N] [--zp]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
import resilient_llm_amd.ops as ops  # noqa: E402
from resilient_llm_amd.ops import ref  # noqa: E402

N, K = 4096, 14336
ROWS = (1, 8, 16, 32, 64)
L3_BYTES = 256 << 20
DEV = "cuda"


def kernel_level(iters, zp):
    G = K // 128
    nq = L3_BYTES // (N * K // 2) + 2
    g = torch.Generator(device=DEV).manual_seed(N + K)
    packed = [torch.randint(-2 ** 31, 2 ** 31 - 1, (N * K // 8,),
                            dtype=torch.int32, device=DEV, generator=g)
              for _ in range(nq)]
    scales = [0.003 * (1 + torch.rand(N, G, device=DEV, generator=g))
              for _ in range(nq)]
    if zp:
        sm = [ref.w4_zp_meta(torch.randint(0, 16, (N, G), dtype=torch.uint8,
                                           device=DEV, generator=g), s.half())
              for s in scales]
        fused_op, plain_op = ops.w4a16_zp_silu_linear, ops.w4a16_zp_linear
    else:
        sm = [s.bfloat16() for s in scales]
        fused_op, plain_op = ops.w4a16_silu_linear, ops.w4a16_linear
    slab = torch.empty(ops.w4a16_plan(N, K)[0] * 64 * N, dtype=torch.float32,
                       device=DEV)
    print(f"{'zp' if zp else 'sym'} N={N} K={K}\n{'M':>3} {'(f) fused us':>13} "
          f"{'(p) silu_mul + linear us':>25} {'p/f':>6}")
    rows = []
    for M in ROWS:
        gus = [(4 * torch.randn(M, 2 * K, device=DEV, generator=g)).bfloat16()
               for _ in range(nq)]

        def fused(i):
            return fused_op(gus[i % nq], packed[i % nq], sm[i % nq], ws=slab)

        def pair(i):
            return plain_op(ops.silu_mul(gus[i % nq]), packed[i % nq],
                            sm[i % nq], ws=slab)

        assert torch.equal(fused(0), pair(0))
        for i in range(10):
            fused(i), pair(i)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
              for _ in range(iters)]
        for i, (a, b, c) in enumerate(ev):
            a.record()
            fused(i)
            b.record()
            pair(i)
            c.record()
        torch.cuda.synchronize()
        f = statistics.median(a.elapsed_time(b) for a, b, _ in ev) * 1e3
        p = statistics.median(b.elapsed_time(c) for _, b, c in ev) * 1e3
        rows.append(dict(M=M, fused_us=f, pair_us=p))
        print(f"{M:3d} {f:13.2f} {p:25.2f} {p / f:6.2f}", flush=True)
    print(json.dumps({"w4a16_silu_zp" if zp else "w4a16_silu": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--zp", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ops.load_extension(required=True)
    kernel_level(args.iters, args.zp)


if __name__ == "__main__":
    main()
