"""Op dispatch: hand-written gfx950 HIP kernels on GPU, fp32 torch
references on CPU.

On a CUDA/ROCm device the HIP extension is REQUIRED — a missing .so
raises immediately rather than silently falling back to eager PyTorch
(the round-end check records which native libraries the GPU tests
actually loaded).  On CPU the ops/ref.py implementations run, which is
what the no-GPU plumbing tests and the gloo multi-process tests use.
"""

from __future__ import annotations

import os
import torch

from . import ref  # noqa: F401

_SO_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_rlli_hip.so")
_loaded = False


class ExtensionMissing(RuntimeError):
    pass


def load_extension(required: bool = False) -> bool:
    """Load the in-tree .so (idempotent).  ``required=True`` (or any GPU
    call) raises if it is absent — no silent eager fallback on GPU."""
    global _loaded
    if _loaded:
        return True
    if os.path.exists(_SO_PATH):
        torch.ops.load_library(_SO_PATH)
        _loaded = True
        return True
    if required:
        raise ExtensionMissing(
            f"HIP extension not built: {_SO_PATH} missing. "
            f"Run `python -m resilient_llm_amd.ops.build`.")
    return False


def extension_loaded() -> bool:
    return _loaded


def _gpu() -> None:
    load_extension(required=True)


# ------------------------------------------------------------------ ops
def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.rmsnorm(x, w, eps)
    return ref.rmsnorm(x, w, eps)


def rmsnorm_residual_(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor,
                      eps: float = 1e-5) -> torch.Tensor:
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.rmsnorm_residual_(x, residual, w, eps)
    return ref.rmsnorm_residual_(x, residual, w, eps)


def rmsnorm_fp8(x, w, eps: float = 1e-5):
    """Fused rmsnorm + per-row fp8-e4m3 quantization -> (q, scales)."""
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.rmsnorm_fp8(x, w, eps)
    return ref.rmsnorm_fp8(x, w, eps)


def rmsnorm_residual_fp8(x, residual, w, eps: float = 1e-5):
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.rmsnorm_residual_fp8(x, residual, w, eps)
    return ref.rmsnorm_residual_fp8(x, residual, w, eps)


def silu_mul_fp8(gate_up):
    if gate_up.is_cuda:
        _gpu()
        return torch.ops.rlli.silu_mul_fp8(gate_up)
    return ref.silu_mul_fp8(gate_up)


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    if gate_up.is_cuda:
        _gpu()
        return torch.ops.rlli.silu_mul(gate_up)
    return ref.silu_mul(gate_up)


def rope_kv_append_(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    positions: torch.Tensor, cos_sin: torch.Tensor,
                    k_cache: torch.Tensor, v_cache: torch.Tensor,
                    slot_mapping: torch.Tensor) -> None:
    if q.is_cuda:
        _gpu()
        torch.ops.rlli.rope_kv_append_(q, k, v, positions, cos_sin,
                                       k_cache, v_cache, slot_mapping)
    else:
        ref.rope_kv_append_(q, k, v, positions, cos_sin, k_cache, v_cache,
                            slot_mapping)


def rope_kv_append_qkv_(qkv: torch.Tensor, positions: torch.Tensor,
                        cos_sin: torch.Tensor, k_cache: torch.Tensor,
                        v_cache: torch.Tensor, slot_mapping: torch.Tensor,
                        n_q: int) -> None:
    """Fused-QKV form: rope + cache append on strided views of the raw
    qkv GEMM output (no .contiguous() copies)."""
    if qkv.is_cuda:
        _gpu()
        torch.ops.rlli.rope_kv_append_qkv_(qkv, positions, cos_sin, k_cache,
                                           v_cache, slot_mapping, n_q)
        return
    T = qkv.shape[0]
    n_kv, _, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    q = qkv[:, :n_q * D].view(T, n_q, D)
    k = qkv[:, n_q * D:(n_q + n_kv) * D].view(T, n_kv, D)
    v = qkv[:, (n_q + n_kv) * D:].view(T, n_kv, D)
    ref.rope_kv_append_(q, k, v, positions, cos_sin, k_cache, v_cache,
                        slot_mapping)


def decode_attn_qkv(qkv: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, block_table: torch.Tensor,
                    seq_lens: torch.Tensor, scale: float,
                    n_q: int) -> torch.Tensor:
    if qkv.is_cuda:
        _gpu()
        return torch.ops.rlli.decode_attn_qkv(qkv, k_cache, v_cache,
                                              block_table, seq_lens, scale, n_q)
    B = qkv.shape[0]
    D = k_cache.shape[3]
    q = qkv[:, :n_q * D].reshape(B, n_q, D)
    out = ref.decode_attn(q, k_cache, v_cache, block_table, seq_lens, scale)
    return out.reshape(B, n_q * D)


def decode_attn_rope_qkv(qkv, positions, cos_sin, k_cache, v_cache,
                         slot_mapping, block_table, seq_lens, scale: float,
                         n_q: int) -> torch.Tensor:
    """Fused decode step: rope(q,k) + cache append + paged attention in
    one kernel on GPU; composed from the unfused reference ops on CPU."""
    if qkv.is_cuda:
        _gpu()
        return torch.ops.rlli.decode_attn_rope_qkv(
            qkv, positions, cos_sin, k_cache, v_cache, slot_mapping,
            block_table, seq_lens, scale, n_q)
    rope_kv_append_qkv_(qkv, positions, cos_sin, k_cache, v_cache,
                        slot_mapping, n_q)
    return decode_attn_qkv(qkv, k_cache, v_cache, block_table, seq_lens,
                           scale, n_q)


def prefill_attn_qkv(qkv: torch.Tensor, cu_seqlens: torch.Tensor,
                     scale: float, n_q: int, n_kv: int,
                     head_dim: int) -> torch.Tensor:
    if qkv.is_cuda:
        _gpu()
        return torch.ops.rlli.prefill_attn_qkv(qkv, cu_seqlens, scale, n_q,
                                               n_kv, head_dim)
    T = qkv.shape[0]
    D = head_dim
    q = qkv[:, :n_q * D].reshape(T, n_q, D)
    k = qkv[:, n_q * D:(n_q + n_kv) * D].reshape(T, n_kv, D)
    v = qkv[:, (n_q + n_kv) * D:].reshape(T, n_kv, D)
    return ref.prefill_attn(q, k, v, cu_seqlens, scale).reshape(T, n_q * D)


def decode_attn(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                block_table: torch.Tensor, seq_lens: torch.Tensor,
                scale: float) -> torch.Tensor:
    if q.is_cuda:
        _gpu()
        return torch.ops.rlli.decode_attn(q, k_cache, v_cache, block_table,
                                          seq_lens, scale)
    return ref.decode_attn(q, k_cache, v_cache, block_table, seq_lens, scale)


def prefill_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 cu_seqlens: torch.Tensor, scale: float) -> torch.Tensor:
    if q.is_cuda:
        _gpu()
        return torch.ops.rlli.prefill_attn(q, k, v, cu_seqlens, scale)
    return ref.prefill_attn(q, k, v, cu_seqlens, scale)


def sample(logits: torch.Tensor, temperatures: torch.Tensor,
           seeds: torch.Tensor, step: int = 0) -> torch.Tensor:
    """Greedy argmax / Gumbel-max temperature sampling; ``seeds`` is a
    per-row int64 tensor (per-request reproducibility), ``step`` a
    uniform step offset mixed in-kernel."""
    if logits.is_cuda:
        _gpu()
        return torch.ops.rlli.sample(logits, temperatures, seeds, step)
    return ref.sample(logits, temperatures, seeds, step)


def sample_constrained(logits: torch.Tensor, rows: torch.Tensor,
                       temperatures: torch.Tensor, seeds: torch.Tensor,
                       step: int, top_k: torch.Tensor, min_p: torch.Tensor,
                       bias_offsets: torch.Tensor, bias_ids: torch.Tensor,
                       bias_vals: torch.Tensor) -> torch.Tensor:
    """Sample rows ``rows`` of ``logits`` under logit_bias / top_k / min_p
    -> int32 tokens [R].  With z = float(logit) + bias: keep z >= the
    k-th largest z (boundary ties stay; k == 0 or k >= vocab is off) and
    z >= z_max + T*ln(min_p) (0 is off), then ``sample``'s own greedy /
    Gumbel-max choice over what is kept.  ``temperatures`` and ``seeds``
    are per logits row (indexed by ``rows[r]``); ``top_k``, ``min_p`` and
    the CSR bias list (``bias_ids`` ascending within a row) are per
    selected row.  The logits are not modified."""
    if logits.is_cuda:
        _gpu()
        return torch.ops.rlli.sample_constrained(
            logits, rows, temperatures, seeds, step, top_k, min_p,
            bias_offsets, bias_ids, bias_vals)
    return ref.sample_constrained(logits, rows, temperatures, seeds, step,
                                  top_k, min_p, bias_offsets, bias_ids,
                                  bias_vals)


def token_logprobs(logits: torch.Tensor, rows: torch.Tensor,
                   tokens: torch.Tensor, k: int):
    """Log-probability of ``tokens[i]`` under row ``rows[i]`` of the RAW
    logits, plus each selected row's ``k`` (0..20) most likely tokens by
    value descending, index ascending on ties -> (chosen_lp [R],
    top_lp [R, k], top_ids [R, k]).  The numbers are the model's own
    distribution: temperature, top-p and penalties do not enter."""
    if logits.is_cuda:
        _gpu()
        return torch.ops.rlli.token_logprobs(logits, rows, tokens, k)
    return ref.token_logprobs(logits, rows, tokens, k)


def kv_copy_blocks_(k_cache: torch.Tensor, v_cache: torch.Tensor,
                    src: torch.Tensor, dst: torch.Tensor) -> None:
    """Fork copy on the paged cache: for every layer l and pair p,
    ``cache[l, dst[p]] = cache[l, src[p]]`` for both [L, NB, H, bs, D]
    caches — in place, bit-exact, one launch, any 1/2/4-byte element.
    ``src`` / ``dst`` are int32 tensors on the cache's device; ``src`` may
    repeat, ``dst`` entries are unique and disjoint from ``src`` (the
    caller's contract).  Every other block is untouched."""
    if k_cache.is_cuda:
        _gpu()
        torch.ops.rlli.kv_copy_blocks_(k_cache, v_cache, src, dst)
    else:
        ref.kv_copy_blocks_(k_cache, v_cache, src, dst)


def lora_shrink(x: torch.Tensor, A: torch.Tensor,
                adapter_idx: torch.Tensor) -> torch.Tensor:
    """Batched multi-adapter LoRA, first half: y[t, r] = sum_k x[t, k] *
    A[a(t), r, k] -> [T, R] f32, with a(t) = ``adapter_idx[t]`` (int32;
    -1 = no adapter: the row does no memory traffic and its y row is
    unspecified on the device).  A is the stack [n_adapters, R, K] with
    R = n_slices * r_max <= 192."""
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.lora_shrink(x, A, adapter_idx)
    return ref.lora_shrink(x, A, adapter_idx)


def lora_expand_add_(out: torch.Tensor, y: torch.Tensor, B: torch.Tensor,
                     scale: torch.Tensor, slices,
                     adapter_idx: torch.Tensor) -> torch.Tensor:
    """Second half, in place on the base GEMM's output: out[t, o] +=
    scale[a] * sum_j y[t, s*r_max + j] * B[a, o, j], rounded once at the
    add; s is the slice of output row o under ``slices`` (<= 3 ascending
    end-exclusive row boundaries, the last == O; q|k|v, gate|up or one
    slice).  B [n_adapters, O, r_max <= 64], scale [n_adapters] f32.
    One writer per element: repeated calls are bit-identical.  Rows with
    adapter_idx -1 are neither read nor written."""
    if out.is_cuda:
        _gpu()
        torch.ops.rlli.lora_expand_add_(out, y, B, scale, list(slices),
                                        adapter_idx)
        return out
    return ref.lora_expand_add_(out, y, B, scale, slices, adapter_idx)


def prefill_paged_attn(qkv, k_cache, v_cache, chunk_row0, chunk_pos0,
                       chunk_nrows, chunk_btrow, block_tables,
                       scale: float, n_q: int) -> torch.Tensor:
    if qkv.is_cuda:
        _gpu()
        return torch.ops.rlli.prefill_paged_attn(
            qkv, k_cache, v_cache, chunk_row0, chunk_pos0, chunk_nrows,
            chunk_btrow, block_tables, scale, n_q)
    return ref.prefill_paged_attn(qkv, k_cache, v_cache, chunk_row0,
                                  chunk_pos0, chunk_nrows, chunk_btrow,
                                  block_tables, scale, n_q)


def skinny_linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Decode-projection GEMM (M<=64): custom MFMA weight-streaming
    kernel on GPU, F.linear on CPU."""
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.skinny_linear(x, w)
    return torch.nn.functional.linear(x, w)


def linear_auto(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Pick the skinny-M kernel when the shape qualifies, else
    hipBLASLt via F.linear."""
    if (x.is_cuda and x.dim() == 2 and 1 <= x.shape[0] <= 64
            and x.shape[1] % 256 == 0 and w.shape[0] % 64 == 0):
        _gpu()
        return torch.ops.rlli.skinny_linear(x, w)
    return torch.nn.functional.linear(x, w)


def skinny2_linear(x: torch.Tensor, w: torch.Tensor,
                   splitk: int = 0) -> torch.Tensor:
    """v2 zero-LDS skinny GEMM (M <= 64); splitk <= 0 = auto."""
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.skinny2_linear(x, w, splitk)
    return torch.nn.functional.linear(x, w)


def skinny2_silu_linear(gu: torch.Tensor, w: torch.Tensor,
                        splitk: int = 0) -> torch.Tensor:
    """Fused SwiGLU + down-proj: (silu(gu[:, :K]) * gu[:, K:]) @ w^T with
    the activation computed inside the GEMM's A-fragment loads — deletes
    the silu_mul launch and its intermediate tensor."""
    if gu.is_cuda:
        _gpu()
        return torch.ops.rlli.skinny2_silu_linear(gu, w, splitk)
    return torch.nn.functional.linear(ref.silu_mul(gu), w)


def w4a16_linear(x: torch.Tensor, packed: torch.Tensor, s: torch.Tensor,
                 splitk: int = 0, out: torch.Tensor | None = None,
                 ws: torch.Tensor | None = None) -> torch.Tensor:
    """Fused int4-weight GEMM for decode rows: out[m, n] = bf16(sum_g
    s[n, g] * sum_{k in g} x[m, k] * q[n, k]), x [M, K] bf16 with
    1 <= M <= 64, ``packed`` / ``s`` from ``ref.w4_pack`` /
    ``ref.quantize_w4`` (group 128 along K; K % 128 == 0, N % 64 == 0).
    Row m depends on row m of x only and is bit-identical for every M;
    no atomics.  ``splitk`` <= 0 picks the K-slicing from (N, K)
    (``w4a16_plan``).  ``out`` [M, N] bf16 is written in full and nothing
    else is, apart from the split-K slab: the first slices*M*N floats of
    ``ws`` when given, else a tensor the op allocates."""
    if x.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((x.shape[0], s.shape[0]), dtype=x.dtype,
                              device=x.device)
        torch.ops.rlli.w4a16_linear_(x, packed, s, splitk, out, ws)
        return out
    y = ref.w4a16_linear(x, packed, s)
    if out is None:
        return y
    out.copy_(y)
    return out


def w4a16_plan(N: int, K: int, splitk: int = 0) -> tuple[int, int]:
    """(slices, k per slice) ``w4a16_linear`` runs with on the GPU: K is
    cut in whole 128-k groups, ceil(groups / slices) per slice."""
    _gpu()
    sk, kps = torch.ops.rlli.w4a16_plan(N, K, splitk)
    return int(sk), int(kps)


def w4_dequant(packed: torch.Tensor, s: torch.Tensor,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 [N, K] = bf16(f32(s) * q) of an int4 weight, into ``out``
    when given (a caller-owned scratch buffer) — the path for more rows
    than the fused kernel takes."""
    if packed.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((s.shape[0], s.shape[1] * ref.W4_GROUP),
                              dtype=torch.bfloat16, device=packed.device)
        torch.ops.rlli.w4_dequant_(packed, s, out)
        return out
    return ref.w4_dequant(packed, s, out)


build_cos_sin = ref.build_cos_sin
