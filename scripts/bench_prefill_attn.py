#!/usr/bin/env python3
"""Microbench: prefill attention at serving shapes — the VALU kernel, the
MFMA in-batch entry, and the MFMA paged entry (32-row chunks over a bf16
and over an fp8 cache holding the same sequence lengths)."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import resilient_llm_amd.ops as ops

BS = 16     # cache block size

def timeit(fn, iters=30, reps=5):
    """Median over ``reps`` windows of ``iters`` launches, each window
    closed by a device synchronise; microseconds per launch."""
    for _ in range(5): fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.monotonic()
        for _ in range(iters): fn()
        torch.cuda.synchronize()
        times.append((time.monotonic() - t0) / iters * 1e6)
    return statistics.median(times)

def paged_case(n_seqs, L, n_kv, D, dtype):
    """Random cache + shuffled block table + 32-row chunk tensors."""
    nb = L // BS
    kc = torch.randn(n_seqs * nb, n_kv, BS, D).to(dtype).cuda()
    vc = torch.randn(n_seqs * nb, n_kv, BS, D).to(dtype).cuda()
    bt = torch.randperm(n_seqs * nb, device="cuda").int().reshape(n_seqs, nb)
    row0 = torch.arange(0, n_seqs * L, 32, dtype=torch.int32, device="cuda")
    return (kc, vc, row0, row0 % L, torch.full_like(row0, 32), row0 // L,
            bt.contiguous())

def main():
    n_q, n_kv, D = 32, 8, 128
    for n_seqs, L in ((64, 128), (16, 512), (4, 2048), (1, 8192)):
        T = n_seqs * L
        width = (n_q + 2 * n_kv) * D
        qkv = torch.randn(T, width, dtype=torch.bfloat16, device="cuda")
        cu = torch.arange(0, T + 1, L, dtype=torch.int32, device="cuda")
        q = qkv[:, :n_q * D].reshape(T, n_q, D).contiguous()
        k = qkv[:, n_q * D:(n_q + n_kv) * D].reshape(T, n_kv, D).contiguous()
        v = qkv[:, (n_q + n_kv) * D:].reshape(T, n_kv, D).contiguous()
        scale = 0.088
        t_m = timeit(lambda: ops.prefill_attn_qkv(qkv, cu, scale, n_q, n_kv, D))
        t_v = timeit(lambda: ops.prefill_attn(q, k, v, cu, scale))
        t_p = {}
        for name, dtype in (("bf16", torch.bfloat16),
                            ("fp8", torch.float8_e4m3fn)):
            case = paged_case(n_seqs, L, n_kv, D, dtype)
            t_p[name] = timeit(
                lambda: ops.prefill_paged_attn(qkv, *case, scale, n_q))
        flops = n_seqs * (L * (L + 1) / 2) * D * 2 * 2 * n_q
        tf = lambda t: f"{t:8.1f} us ({flops/t/1e6:6.1f} TF)"
        print(f"{n_seqs}x{L}: VALU {tf(t_v)} MFMA {tf(t_m)}  x{t_v/t_m:.2f}  "
              f"paged bf16 {tf(t_p['bf16'])} paged fp8 {tf(t_p['fp8'])}",
              flush=True)

if __name__ == "__main__":
    main()
