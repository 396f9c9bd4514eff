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


def qk_norm_rope_kv_append_qkv_(qkv: torch.Tensor, q_norm_w: torch.Tensor,
                                k_norm_w: torch.Tensor, eps: float,
                                positions: torch.Tensor,
                                cos_sin: torch.Tensor, k_cache: torch.Tensor,
                                v_cache: torch.Tensor,
                                slot_mapping: torch.Tensor, n_q: int) -> None:
    """``rope_kv_append_qkv_`` for models with a q/k norm (Qwen3): every q
    head and k head of the raw qkv rows goes through RMSNorm over its
    head_dim values (``q_norm_w`` / ``k_norm_w``, [head_dim], shared by all
    heads; the normalised value stays in f32) and is then rotated, rounded
    to bf16 and appended as there.
    v is untouched.  One kernel; head_dim 64 or 128."""
    if qkv.is_cuda:
        _gpu()
        torch.ops.rlli.qk_norm_rope_kv_append_qkv_(
            qkv, q_norm_w, k_norm_w, eps, positions, cos_sin, k_cache,
            v_cache, slot_mapping, n_q)
        return
    T = qkv.shape[0]
    n_kv, D = k_cache.shape[1], k_cache.shape[3]
    q = qkv[:, :n_q * D].view(T, n_q, D)
    k = qkv[:, n_q * D:(n_q + n_kv) * D].view(T, n_kv, D)
    v = qkv[:, (n_q + n_kv) * D:].view(T, n_kv, D)
    ref.qk_norm_rope_kv_append_(q, k, v, q_norm_w, k_norm_w, eps, positions,
                                cos_sin, k_cache, v_cache, slot_mapping)


def decode_attn_qknorm_rope_qkv(qkv, q_norm_w, k_norm_w, eps: float,
                                positions, cos_sin, k_cache, v_cache,
                                slot_mapping, block_table, seq_lens,
                                scale: float, n_q: int) -> torch.Tensor:
    """``decode_attn_rope_qkv`` with the q/k norm of
    ``qk_norm_rope_kv_append_qkv_`` applied in registers before the
    rotation: still one kernel on GPU (cache block size 16 only, the
    engine's); composed from the unfused ops on CPU."""
    if qkv.is_cuda:
        _gpu()
        return torch.ops.rlli.decode_attn_qknorm_rope_qkv(
            qkv, q_norm_w, k_norm_w, eps, positions, cos_sin, k_cache,
            v_cache, slot_mapping, block_table, seq_lens, scale, n_q)
    qk_norm_rope_kv_append_qkv_(qkv, q_norm_w, k_norm_w, eps, positions,
                                cos_sin, k_cache, v_cache, slot_mapping, n_q)
    return decode_attn_qkv(qkv, k_cache, v_cache, block_table, seq_lens,
                           scale, n_q)


def shared_prefix_chunks(tiles: int, n_kv: int, kv_tiles: int) -> int:
    """Chunks of the shared prefix per (row tile, kv-head) that fill the
    device: what a ``decode_attn_shared_qkv`` plan's workspace is sized
    with when the longest prefix spans ``kv_tiles`` 64-token tiles."""
    _gpu()
    return int(torch.ops.rlli.shared_prefix_chunks(tiles, n_kv, kv_tiles))


def decode_attn_shared_qkv(qkv: torch.Tensor, k_cache: torch.Tensor,
                           v_cache: torch.Tensor, block_table: torch.Tensor,
                           seq_lens: torch.Tensor, plan, scale: float,
                           n_q: int) -> torch.Tensor:
    """``decode_attn_qkv`` for a batch whose rows share leading physical
    KV blocks: each group's shared run is read once (MFMA, f32 partials
    into the plan's workspace), then every row walks its private blocks
    and folds its partials in.  ``plan`` = (n_shared [B] shared tokens
    per row, 0 = in no group; row_tile [B]; row_slot [B]; tile_rows
    [T, 64/GROUP] member rows, -1 padded; tile_blocks [T]; tile_bt_row
    [T]; ws_acc [T, n_kv, chunks, 64, D] f32; ws_ml [T, n_kv, chunks, 64,
    2] f32) — int32 device tensors from ``engine.kv_cache`` plus the
    workspace, whose third dimension is the chunk count the call runs
    with.  bf16 cache, block size 16, head_dim 128, GQA group 4 or 8.
    Mathematically ``decode_attn_qkv``; P is rounded to bf16 in the
    shared phase.  On CPU tensors it is ``decode_attn_qkv``."""
    if qkv.is_cuda:
        _gpu()
        return torch.ops.rlli.decode_attn_shared_qkv(
            qkv, k_cache, v_cache, block_table, seq_lens, list(plan), scale,
            n_q)
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


def sample_nucleus_max_history() -> int:
    """Largest history capacity (tokens per slot) ``sample_nucleus``
    takes: its LDS count table holds twice as many entries.  The loaded
    extension's own limit when there is one, else the reference's."""
    if _loaded:
        return int(torch.ops.rlli.sample_nucleus_max_history())
    return ref.NUCLEUS_MAX_HISTORY


def sample_nucleus(logits: torch.Tensor, rows: torch.Tensor,
                   temperatures: torch.Tensor, seeds: torch.Tensor,
                   step: int, top_k: torch.Tensor, min_p: torch.Tensor,
                   top_p: torch.Tensor, presence: torch.Tensor,
                   frequency: torch.Tensor, bias_offsets: torch.Tensor,
                   bias_ids: torch.Tensor, bias_vals: torch.Tensor,
                   hist_slot: torch.Tensor, history: torch.Tensor,
                   hist_len: torch.Tensor, append: bool,
                   check_slots: bool = True) -> torch.Tensor:
    """``sample_constrained`` plus nucleus (top_p) filtering and presence /
    frequency penalties for rows ``rows`` of ``logits`` -> int32 tokens [R].

    ``history`` int32 [n_slots, cap] holds one token history per slot,
    ``hist_len`` int32 [n_slots] its length; selected row r uses slot
    ``hist_slot[r]`` (-1: none; slots of one call are distinct).  With
    c(t) the count of t in that history (ids outside the vocab ignored),

      z(t) = float(logit) - (presence[r] + frequency[r] * c(t)) [c(t) > 0]
             + bias(t)                       (fp32, in this order)

    Greedy rows (T <= 0) take arg-max z, lowest index on ties.  Sampled
    rows keep z >= the k-th largest z and z >= z_max + T*ln(min_p) as
    ``sample_constrained`` does, then the nucleus over the survivors: with
    w = exp((z - z_max)/T) and W their total weight, t stays iff the
    weight of survivors with z strictly above z(t) is < top_p[r] * W —
    the smallest prefix whose mass reaches top_p, with every token equal
    to the boundary value kept (top_p <= 0 or >= 1 is off).  The draw is
    ``sample``'s Gumbel-max over what is kept, keyed by (seed, step, index)
    alike: a row with no penalty and top_p off gets ``sample_constrained``'s
    token.  With ``append`` the chosen token is stored at
    ``history[slot, hist_len[slot]]`` and the length grows by one, unless
    the slot is full.  The logits are not modified.  ``check_slots``
    validates the ``hist_slot`` values on the host, which synchronizes; a
    caller that built them itself may pass False."""
    if logits.is_cuda:
        _gpu()
        return torch.ops.rlli.sample_nucleus(
            logits, rows, temperatures, seeds, step, top_k, min_p, top_p,
            presence, frequency, bias_offsets, bias_ids, bias_vals,
            hist_slot, history, hist_len, append, check_slots)
    return ref.sample_nucleus(logits, rows, temperatures, seeds, step, top_k,
                              min_p, top_p, presence, frequency,
                              bias_offsets, bias_ids, bias_vals, hist_slot,
                              history, hist_len, append)


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


def w4a16_zp_linear(x: torch.Tensor, packed: torch.Tensor,
                    meta: torch.Tensor, splitk: int = 0,
                    out: torch.Tensor | None = None,
                    ws: torch.Tensor | None = None) -> torch.Tensor:
    """``w4a16_linear`` for zero-point (AWQ) weights: out[m, n] =
    bf16(sum_g s[n, g] * sum_{k in g} x[m, k] * (u[n, k] - z[n, g])),
    ``packed`` the nibbles u in ``ref.w4_pack`` order, ``meta`` int32
    [N, K/128] from ``ref.w4_zp_meta`` (or both from ``awq_repack``).
    Shapes, slicing, ``out`` / ``ws`` and the row contract are those of
    ``w4a16_linear``."""
    if x.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((x.shape[0], meta.shape[0]), dtype=x.dtype,
                              device=x.device)
        torch.ops.rlli.w4a16_zp_linear_(x, packed, meta, splitk, out, ws)
        return out
    y = ref.w4a16_zp_linear(x, packed, meta)
    if out is None:
        return y
    out.copy_(y)
    return out


def _check_w4_silu_cpu(gu: torch.Tensor, sm: torch.Tensor, splitk: int,
                       ws: torch.Tensor | None) -> None:
    """What the device ops check about ``gu`` and ``ws``, for CPU tensors
    (``sm`` is s or meta, [N, K/128])."""
    N, G = sm.shape
    K = G * ref.W4_GROUP
    if gu.dtype != torch.bfloat16 or gu.dim() != 2 or gu.stride(1) != 1:
        raise ValueError("gu must be bf16 [M, 2K] with unit inner stride")
    M, width = gu.shape
    if width % 2 or width != 2 * K:
        raise ValueError(f"gu must be [M, 2K] = [M, {2 * K}], got width "
                         f"{width}")
    if not 1 <= M <= 64:
        raise ValueError(f"w4a16_silu_linear needs 1 <= M <= 64, got {M}")
    if ws is not None:
        # w4a16_plan: whole groups per slice, no empty slice
        panels = N // 64
        sk = (min(splitk, G) if splitk > 0 else
              min(max(1, -(-1024 // panels)), max(1, G // 4)))
        slices = -(-G // -(-G // sk))
        if slices > 1 and (ws.dtype != torch.float32
                           or ws.numel() < slices * M * N):
            raise ValueError(f"ws must be f32 with >= slices*M*N = "
                             f"{slices * M * N} elements")


def w4a16_silu_linear(gu: torch.Tensor, packed: torch.Tensor,
                      s: torch.Tensor, splitk: int = 0,
                      out: torch.Tensor | None = None,
                      ws: torch.Tensor | None = None) -> torch.Tensor:
    """SwiGLU fused into ``w4a16_linear`` (the int4 decode down
    projection): out[m, n] = bf16(sum_g s[n, g] * sum_{k in g} a[m, k] *
    q[n, k]) with a[m, k] = bf16(silu(gu[m, k]) * gu[m, K + k]) built in
    the kernel's A fragments from ``gu`` [M, 2K] bf16, the packed gate|up
    rows, 1 <= M <= 64.  Bit-identical to ``w4a16_linear(silu_mul(gu),
    packed, s)`` for every M, without that launch and its [M, K]
    intermediate; ``packed`` / ``s``, slicing, ``out`` / ``ws`` and the row
    contract are those of ``w4a16_linear``."""
    if gu.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((gu.shape[0], s.shape[0]), dtype=gu.dtype,
                              device=gu.device)
        torch.ops.rlli.w4a16_silu_linear_(gu, packed, s, splitk, out, ws)
        return out
    _check_w4_silu_cpu(gu, s, splitk, ws)
    y = ref.w4a16_silu_linear(gu, packed, s)
    if out is None:
        return y
    out.copy_(y)
    return out


def w4a16_zp_silu_linear(gu: torch.Tensor, packed: torch.Tensor,
                         meta: torch.Tensor, splitk: int = 0,
                         out: torch.Tensor | None = None,
                         ws: torch.Tensor | None = None) -> torch.Tensor:
    """``w4a16_silu_linear`` for zero-point (AWQ) weights: bit-identical
    to ``w4a16_zp_linear(silu_mul(gu), packed, meta)``."""
    if gu.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((gu.shape[0], meta.shape[0]), dtype=gu.dtype,
                              device=gu.device)
        torch.ops.rlli.w4a16_zp_silu_linear_(gu, packed, meta, splitk, out,
                                             ws)
        return out
    _check_w4_silu_cpu(gu, meta, splitk, ws)
    y = ref.w4a16_zp_silu_linear(gu, packed, meta)
    if out is None:
        return y
    out.copy_(y)
    return out


def w4_zp_dequant(packed: torch.Tensor, meta: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 [N, K] = bf16(f32(s) * (u - z)) of a zero-point int4 weight,
    into ``out`` when given."""
    if packed.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((meta.shape[0], meta.shape[1] * ref.W4_GROUP),
                              dtype=torch.bfloat16, device=packed.device)
        torch.ops.rlli.w4_zp_dequant_(packed, meta, out)
        return out
    return ref.w4_zp_dequant(packed, meta, out)


def awq_repack(qweight: torch.Tensor, qzeros: torch.Tensor,
               scales: torch.Tensor, packed: torch.Tensor,
               meta: torch.Tensor, col_offset: int = 0) -> None:
    """One projection of an AutoAWQ checkpoint (GEMM layout, 4 bits, group
    128: ``qweight`` int32 [K, N/8], ``qzeros`` int32 [K/128, N/8],
    ``scales`` fp16 [K/128, N]) into output columns ``col_offset`` ..
    ``col_offset + N`` of ``packed`` int32 [N_total*K/8] and ``meta`` int32
    [N_total, K/128]: q/k/v and gate/up repack straight into their slice
    of the fused tensors.  N and col_offset are multiples of 64; nothing
    outside the slice is written."""
    if qweight.is_cuda:
        _gpu()
        torch.ops.rlli.awq_repack_(qweight, qzeros, scales, packed, meta,
                                   col_offset)
        return
    ref.awq_repack(qweight, qzeros, scales, packed, meta, col_offset)


def w4a16_tiled_linear(x: torch.Tensor, packed: torch.Tensor,
                       s: torch.Tensor, splitk: int = 0,
                       out: torch.Tensor | None = None,
                       ws: torch.Tensor | None = None) -> torch.Tensor:
    """``w4a16_linear`` for 1 <= M <= 256 rows (decode batches past 64):
    out[m, n] = bf16(sum_g s[n, g] * sum_{k in g} x[m, k] * q[n, k]) on the
    same ``packed`` / ``s`` tensors (K % 128 == 0, N % 64 == 0).  One
    workgroup of ceil(M / 64) waves per 64-column panel x K-slice reads
    the packed weight once and shares it through LDS; no bf16 weight is
    ever written.  The scale multiplies the group's f32 partial sum, as in
    ``w4a16_linear``.  Row m depends on row m of x only; the K-slicing
    (``w4a16_tiled_plan``; ``splitk`` <= 0 picks it) depends on (N, K)
    only, so a row's bits do not depend on M; no atomics.  ``out`` [M, N]
    bf16 is written in full and nothing else is, apart from the split-K
    slab: the first slices*M*N floats of ``ws`` when given, else a tensor
    the op allocates — with ``out`` and ``ws`` given it allocates
    nothing."""
    if x.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((x.shape[0], s.shape[0]), dtype=x.dtype,
                              device=x.device)
        torch.ops.rlli.w4a16_tiled_linear_(x, packed, s, splitk, out, ws)
        return out
    y = ref.w4a16_linear(x, packed, s)
    if out is None:
        return y
    out.copy_(y)
    return out


def w4a16_zp_tiled_linear(x: torch.Tensor, packed: torch.Tensor,
                          meta: torch.Tensor, splitk: int = 0,
                          out: torch.Tensor | None = None,
                          ws: torch.Tensor | None = None) -> torch.Tensor:
    """``w4a16_tiled_linear`` for zero-point (AWQ) weights: out[m, n] =
    bf16(sum_g s[n, g] * sum_{k in g} x[m, k] * (u[n, k] - z[n, g])) on
    the ``packed`` / ``meta`` tensors of ``w4a16_zp_linear``, 1 <= M <=
    256.  Shapes, slicing, ``out`` / ``ws`` and the row contract are those
    of ``w4a16_tiled_linear``."""
    if x.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((x.shape[0], meta.shape[0]), dtype=x.dtype,
                              device=x.device)
        torch.ops.rlli.w4a16_zp_tiled_linear_(x, packed, meta, splitk, out,
                                              ws)
        return out
    y = ref.w4a16_zp_linear(x, packed, meta)
    if out is None:
        return y
    out.copy_(y)
    return out


def w4a16_tiled_plan(N: int, K: int, splitk: int = 0) -> tuple[int, int]:
    """(slices, k per slice) the tiled ops run with on the GPU: K is cut
    in whole 128-k groups, ceil(groups / slices) per slice, no empty
    slice; a function of (N, K) only."""
    _gpu()
    sk, kps = torch.ops.rlli.w4a16_tiled_plan(N, K, splitk)
    return int(sk), int(kps)


def w4a16_wide_linear(x: torch.Tensor, packed: torch.Tensor,
                      s: torch.Tensor, splitk: int = 0,
                      out: torch.Tensor | None = None,
                      ws: torch.Tensor | None = None) -> torch.Tensor:
    """``w4a16_linear`` for 1 <= M <= 512 rows (mixed steps past the 256
    of the tiled op): out[m, n] = bf16(sum_g s[n, g] * sum_{k in g}
    x[m, k] * q[n, k]) on the same ``packed`` / ``s`` tensors (K % 128 ==
    0, N % 128 == 0).  One workgroup of four waves per 128-column panel x
    128-row block x K-slice converts the packed weight to bf16 once, on
    its way into LDS; no bf16 weight is written to memory.  The scale
    multiplies the group's f32 partial sum, as in ``w4a16_linear``.  Row m
    depends on row m of x only; the K-slicing (``w4a16_wide_plan``;
    ``splitk`` <= 0 picks it) depends on (N, K) only, so a row's bits do
    not depend on M; no atomics.  ``out`` [M, N] bf16 is written in full
    and nothing else is, apart from the split-K slab: the first
    slices*M*N floats of ``ws`` when given, else a tensor the op
    allocates — with ``out`` and ``ws`` given it allocates nothing."""
    if x.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((x.shape[0], s.shape[0]), dtype=x.dtype,
                              device=x.device)
        torch.ops.rlli.w4a16_wide_linear_(x, packed, s, splitk, out, ws)
        return out
    y = ref.w4a16_linear(x, packed, s)
    if out is None:
        return y
    out.copy_(y)
    return out


def w4a16_zp_wide_linear(x: torch.Tensor, packed: torch.Tensor,
                         meta: torch.Tensor, splitk: int = 0,
                         out: torch.Tensor | None = None,
                         ws: torch.Tensor | None = None) -> torch.Tensor:
    """``w4a16_wide_linear`` for zero-point (AWQ) weights: out[m, n] =
    bf16(sum_g s[n, g] * sum_{k in g} x[m, k] * (u[n, k] - z[n, g])) on
    the ``packed`` / ``meta`` tensors of ``w4a16_zp_linear``, 1 <= M <=
    512.  Shapes, slicing, ``out`` / ``ws`` and the row contract are those
    of ``w4a16_wide_linear``."""
    if x.is_cuda:
        _gpu()
        if out is None:
            out = torch.empty((x.shape[0], meta.shape[0]), dtype=x.dtype,
                              device=x.device)
        torch.ops.rlli.w4a16_zp_wide_linear_(x, packed, meta, splitk, out,
                                             ws)
        return out
    y = ref.w4a16_zp_linear(x, packed, meta)
    if out is None:
        return y
    out.copy_(y)
    return out


def w4a16_wide_plan(N: int, K: int, splitk: int = 0) -> tuple[int, int]:
    """(slices, k per slice) the wide ops run with on the GPU: K is cut
    in whole 128-k groups, ceil(groups / slices) per slice, no empty
    slice; a function of (N, K) only."""
    _gpu()
    sk, kps = torch.ops.rlli.w4a16_wide_plan(N, K, splitk)
    return int(sk), int(kps)


def moe_route(router_logits: torch.Tensor, k: int, renorm: bool = True
              ) -> tuple[torch.Tensor, torch.Tensor]:
    """Softmax-top-k router of a Mixture-of-Experts layer: (ids [T, k]
    int32, w [T, k] f32) from ``router_logits`` [T, E] bf16.  ids are the k
    largest logits of the row in descending order, ties to the lower expert
    index, chosen on the logit values (``ref.moe_route``'s stable sort); w
    is the f32 softmax over all E at those ids, divided by their sum with
    ``renorm``.  2 <= E <= 256, 1 <= k <= min(E, 8).  A row holding NaN or
    Inf still yields k distinct ids in [0, E) (NaN counts as the lowest
    value); its weights are then not finite."""
    T, E = router_logits.shape
    if not 2 <= E <= 256 or not 1 <= k <= min(E, 8):
        raise ValueError(f"moe_route needs 2 <= E <= 256 and 1 <= k <= "
                         f"min(E, 8), got E={E} k={k}")
    if router_logits.is_cuda:
        _gpu()
        return torch.ops.rlli.moe_route(router_logits, k, renorm)
    return ref.moe_route(router_logits, k, renorm)


def moe_mlp(x: torch.Tensor, ids: torch.Tensor, w: torch.Tensor,
            w_gate_up: torch.Tensor, w_down: torch.Tensor,
            row_tile: int = 0) -> torch.Tensor:
    """Sparse SwiGLU MLP: out[t] = bf16(sum_j w[t, j] * Wd[e] · bf16(silu(
    Wg[e] · x[t]) * (Wu[e] · x[t]))) with e = ids[t, j], summed in slot
    order.  x [T, H] bf16, ids / w [T, k] from ``moe_route``, w_gate_up
    [E, 2I, H] (gate | up rows), w_down [E, H, I]; H % 64 == 0 and
    I % 64 == 0.  On the GPU: an alignment kernel sorts the (token, slot)
    pairs by expert into row tiles of 16 or 64 rows (``row_tile`` = 0
    picks from T, k and E), a grouped GEMM computes gate and up with SwiGLU
    in its epilogue, a second one the down projection in f32, and a
    combine kernel the weighted sum.  Nothing is read back to the host, so
    the op captures into a graph; no float atomics, so two calls agree bit
    for bit.  Only the experts some row chose are read, and an id outside
    [0, E) contributes nothing.  The workspaces are allocated inside."""
    H, I = x.shape[1], w_down.shape[2]
    if H % 64 or I % 64:
        raise ValueError(f"moe_mlp needs H % 64 == 0 and I % 64 == 0, got "
                         f"H={H} I={I}")
    if (w_gate_up.shape[1:] != (2 * I, H) or w_down.shape[1] != H
            or w_down.shape[0] != w_gate_up.shape[0]
            or ids.shape[0] != x.shape[0] or w.shape != ids.shape):
        raise ValueError("moe_mlp: x [T, H], ids / w [T, k], w_gate_up "
                         "[E, 2I, H], w_down [E, H, I] do not fit")
    if x.is_cuda:
        _gpu()
        return torch.ops.rlli.moe_mlp(x, ids, w, w_gate_up, w_down, row_tile)
    return ref.moe_mlp(x, ids, w, w_gate_up, w_down)


build_cos_sin = ref.build_cos_sin
