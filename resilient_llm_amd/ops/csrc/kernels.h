// Launch-function declarations: pure-HIP translation units (one per
// kernel family) export these; ext.cpp (the only file that includes
// torch headers) validates tensors and calls them.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rlli {

// y = rmsnorm(x) * w           (residual == nullptr)
// r += x; y = rmsnorm(r) * w   (fused residual-add form)
void launch_rmsnorm(const uint16_t* x, uint16_t* residual, const uint16_t* w,
                    uint16_t* y, int rows, int dim, float eps,
                    hipStream_t stream);

// out[t, i] = silu(gu[t, i]) * gu[t, I + i]   for packed gate|up rows
void launch_silu_mul(const uint16_t* gate_up, uint16_t* out, int rows,
                     int inter, hipStream_t stream);

// In-place RoPE (NeoX-interleaved-halves style) on q and k, then scatter
// k/v into the paged cache at slot_mapping[t].
// q/k/v may be strided slices of one fused [T, (n_q+2*n_kv)*D] qkv
// tensor: *_stride is the per-token element stride of each view.
// Cache pointers are void*: the paged cache stores bf16 (default) or
// OCP fp8-e4m3 (cache_fp8) — see common.h cache codecs.
// FP8-activation emitters for the quantized-weight GEMM path
// (rowwise torch._scaled_mm consumers): normed / activated rows out as
// fp8-e4m3 + one dequant scale per row.
void launch_rmsnorm_fp8(const uint16_t* x, uint16_t* residual,
                        const uint16_t* w, uint8_t* y8, float* scales,
                        int rows, int dim, float eps, hipStream_t stream);
void launch_silu_mul_fp8(const uint16_t* gate_up, uint8_t* out8,
                         float* scales, int rows, int inter,
                         hipStream_t stream);

void launch_rope_kv_append(
    uint16_t* q, uint16_t* k, uint16_t* v,
    const int32_t* positions, const float* cos_sin,   // [max_pos, head_dim]
    void* k_cache, void* v_cache,
    const int32_t* slot_mapping,
    int tokens, int n_q_heads, int n_kv_heads, int head_dim,
    int block_size, int q_stride, int kv_stride, bool cache_fp8,
    hipStream_t stream);

// Split-K factor for decode attention (flash-decode): >1 when
// batch*n_kv_heads workgroups cannot fill 256 CUs.  The caller sizes
// the f32 scratch as [batch*n_kv*n_split*group*head_dim] (part_out)
// and [batch*n_kv*n_split*group*2] (part_ml) and passes both; n_split=1
// (or null scratch) is the classic single-workgroup-per-(seq,head) path.
int decode_attn_n_split(int batch, int n_kv_heads);

// Paged GQA decode attention: one new q token per sequence.
// Contract: cache slots past seq_len must hold finite values (masked
// tokens weigh p = 0 but their V is still multiplied, so 0 * NaN/Inf
// would propagate; a zero-initialised cache only ever receives finite
// values).
void launch_decode_attn(
    const uint16_t* q,                 // [batch, n_q_heads, head_dim]
    const void* k_cache,               // [blocks, n_kv, block_size, head_dim]
    const void* v_cache,
    const int32_t* block_table,        // [batch, max_blocks]
    const int32_t* seq_lens,           // [batch]
    uint16_t* out,                     // [batch, n_q_heads, head_dim]
    int batch, int n_q_heads, int n_kv_heads, int head_dim,
    int block_size, int max_blocks, float scale, int q_stride,
    int n_split, float* part_out, float* part_ml, bool cache_fp8,
    hipStream_t stream);

// Fused decode: rope(q,k) + cache append + paged attention in ONE
// kernel (decode path; qkv is the raw fused GEMM output).
void launch_decode_attn_fused(
    const uint16_t* qkv, void* k_cache, void* v_cache,
    const int32_t* block_table, const int32_t* seq_lens,
    const int32_t* positions, const float* cos_sin,
    const int32_t* slot_mapping, uint16_t* out, int batch, int n_q_heads,
    int n_kv_heads, int head_dim, int block_size, int max_blocks,
    float scale, int qkv_stride, int n_split, float* part_out,
    float* part_ml, bool cache_fp8, hipStream_t stream);

// Varlen causal prefill attention over in-batch q/k/v.
void launch_prefill_attn(
    const uint16_t* q, const uint16_t* k, const uint16_t* v,
    const int32_t* cu_seqlens,         // [n_seqs + 1]
    uint16_t* out,
    int n_seqs, int total_tokens, int n_q_heads, int n_kv_heads,
    int head_dim, float scale, int q_stride, int kv_stride,
    hipStream_t stream);

// MFMA varlen causal prefill attention, K/V read from the fused in-batch
// qkv tensor.  Shares its tile body with launch_prefill_paged
// (prefill_mfma.hip); only the K/V source differs.
void launch_prefill_mfma(const uint16_t* qkv, const int32_t* chunk_t0,
                         const int32_t* chunk_seq_start,
                         const int32_t* chunk_seq_end, uint16_t* out,
                         int n_chunks, int n_kv_heads, int group,
                         int head_dim, int qkv_stride, float scale,
                         hipStream_t stream);

// MFMA chunked-prefill attention, K/V read from the paged cache (bf16 or
// fp8) through block tables: chunked prefill and mixed batches.  The same
// tile body as launch_prefill_mfma.
void launch_prefill_paged(const uint16_t* qkv, const void* k_cache,
                          const void* v_cache, const int32_t* chunk_row0,
                          const int32_t* chunk_pos0,
                          const int32_t* chunk_nrows,
                          const int32_t* chunk_btrow,
                          const int32_t* block_tables, uint16_t* out,
                          int n_chunks, int n_kv_heads, int group,
                          int head_dim, int qkv_stride, int max_blocks,
                          int block_size, float scale, bool cache_fp8,
                          hipStream_t stream);

// Skinny-M GEMM (decode projections): out[M,N] = x[M,K] @ W[N,K]^T.
// ws is a [splitk, M, N] f32 workspace (unused when splitk == 1).
// v2: zero-LDS one-wave-per-16-columns register-dataflow skinny GEMM
// (skinny2.hip); ws is the [splitk, M, N] f32 slab when splitk > 1.
void launch_skinny2(const uint16_t* x, const uint16_t* w, float* ws,
                    uint16_t* out, int M, int N, int K, int splitk,
                    hipStream_t stream);
// silu(g)*u fused into the A-fragment path: gu is [M, 2K] (gate|up).
void launch_skinny2_silu(const uint16_t* gu, const uint16_t* w, float* ws,
                         uint16_t* out, int M, int N, int K, int splitk,
                         hipStream_t stream);

// W4A16 (w4a16.hip): int4 group-quantized weights (group 128 along K,
// symmetric, bf16 scales s[N, K/128]) in the fragment-order packing of
// ops/ref.py w4_pack; K % 128 == 0, N % 64 == 0.
//   launch_w4a16: out[M,N] = bf16(sum_g s * sum_{k in g} x * q), M <= 64;
//     ws is the [splitk, M, N] f32 slab when splitk > 1.  w4a16_plan
//     gives the slicing (whole groups per slice, a function of N and K
//     only); splitk_req <= 0 picks the grid-fill heuristic.
//   launch_w4_dequant: out[N,K] = bf16(f32(s) * q).
void w4a16_plan(int N, int K, int splitk_req, int* splitk,
                int* grp_per_slice);
void launch_w4a16(const uint16_t* x, const uint32_t* packed,
                  const uint16_t* s, float* ws, uint16_t* out, int M, int N,
                  int K, int splitk, int grp_per_slice, hipStream_t stream);
void launch_w4_dequant(const uint32_t* packed, const uint16_t* s,
                       uint16_t* out, int N, int K, hipStream_t stream);

void launch_skinny_gemm(const uint16_t* x, const uint16_t* w, float* ws,
                        uint16_t* out, int M, int N, int K, int splitk,
                        hipStream_t stream);

// Diagnostic: pure nt-stream of W at skinny_gemm geometry.
void launch_stream_probe(const uint16_t* w, float* sink, int N, int K,
                         int splitk, hipStream_t stream);

// Fused sampling: greedy argmax when temperature[i] == 0, else Gumbel-max
// sampling of softmax(logits / temperature[i]) with an in-kernel counter
// hash RNG keyed on (seed, row, column) — no 32 MB random tensor per step.
int sample_n_split(int batch);       // phase-A split factor (1 = single)
void launch_sample(
    const uint16_t* logits,            // [batch, vocab] bf16
    const float* temperatures,         // [batch]
    const uint64_t* seeds,             // [batch] per-request seeds
    uint64_t step,                     // per-sequence step counter (mixed in)
    int32_t* out_tokens,               // [batch]
    int batch, int vocab,
    uint64_t* partials, int n_split,   // [batch, n_split] workspace
    hipStream_t stream);

// Constrained sampling of selected rows: z = float(logit) + bias, keep
// z >= k-th largest z (ties stay; k == 0 or k >= vocab: off) and
// z >= z_max + T*ln(min_p) (0: off), then the sampler's own Gumbel-max /
// greedy arg-max over what is kept.  temperatures/seeds are indexed by
// rows[r]; top_k, min_p and the CSR bias list (ids ascending per row) by
// r.  The logits are only read; no workspace (sampling.hip).
int sample_constrained_max_vocab();
void launch_sample_constrained(
    const uint16_t* logits,            // [batch, vocab] bf16
    const int32_t* rows,               // [n_rows] row indices into logits
    const float* temperatures,         // [batch]
    const uint64_t* seeds,             // [batch]
    uint64_t step,
    const int32_t* top_k,              // [n_rows]
    const float* min_p,                // [n_rows]
    const int32_t* bias_offsets,       // [n_rows + 1]
    const int32_t* bias_ids,           // [n_bias_total]
    const float* bias_vals,            // [n_bias_total]
    int n_bias_total,
    int32_t* out_tokens,               // [n_rows]
    int n_rows, int vocab, hipStream_t stream);

// Fused log-softmax value of one emitted token per selected row plus the
// row's k most likely tokens (value descending, index ascending on ties),
// computed on the RAW logits — one pass over the selected rows, nothing
// vocab-wide written (logprobs.hip).
int logprobs_n_split(int rows, int vocab);   // phase-A split factor
void launch_token_logprobs(
    const uint16_t* logits,            // [batch, vocab] bf16
    const int32_t* rows,               // [n_rows] row indices into logits
    const int32_t* tokens,             // [n_rows] emitted token per row
    float* chosen_lp,                  // [n_rows]
    float* top_lp,                     // [n_rows, k]
    int32_t* top_ids,                  // [n_rows, k]
    int n_rows, int vocab, int k,
    float* stats,                      // [n_rows, n_split, 2] workspace
    uint64_t* cand,                    // [n_rows, n_split, k] workspace
    int n_split, hipStream_t stream);

// Paged-cache block copy for forked sequences: for every layer l and pair
// p, cache[l, dst[p]] = cache[l, src[p]] for K and V in one launch, as
// raw bytes (chunk_bytes = H*bs*D*elt, a multiple of 16).  dst ids are
// unique and disjoint from src ids (src may repeat); ids are not
// validated on the device (kv_copy.hip).
void launch_kv_copy_blocks(void* k_cache, void* v_cache, const int32_t* src,
                           const int32_t* dst, int n_pairs, int n_layers,
                           int64_t num_blocks, int64_t chunk_bytes,
                           hipStream_t stream);

// Batched multi-adapter LoRA next to the base GEMM (lora.hip): token row
// t uses adapter adapter_idx[t]; -1 (or an index outside the stack) means
// no adapter and the row is neither read nor written.
//   shrink: y[t, r] = sum_k x[t, k] * A[a, r, k]                (f32)
//   expand: out[t, o] = bf16(float(out[t, o]) + scale[a]
//                       * sum_j y[t, s*r_max + j] * B[a, o, j])
// s = the slice of output row o under the ascending end-exclusive
// slice_ends (host array of n_slices <= 3 entries, the last one == O);
// R = n_slices * r_max <= 192, r_max <= 64.
void launch_lora_shrink(const uint16_t* x,            // [T, K] bf16
                        const uint16_t* A,            // [n_adapters, R, K]
                        const int32_t* adapter_idx,   // [T]
                        float* y,                     // [T, R]
                        int T, int n_adapters, int R, int K,
                        hipStream_t stream);
void launch_lora_expand_add(uint16_t* out,            // [T, O] bf16, in place
                            const float* y,           // [T, R]
                            const uint16_t* B,        // [n_adapters, O, r_max]
                            const float* scale,       // [n_adapters]
                            const int32_t* adapter_idx,
                            int T, int n_adapters, int O, int r_max,
                            int n_slices, const int* slice_ends,
                            hipStream_t stream);

}  // namespace rlli
