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

// launch_rope_kv_append with a per-head RMSNorm on q and on k between the
// projection and the rotation (Qwen3): n = x * rsqrt(mean(x^2) + eps) * w
// in f32, w = q_norm_w / k_norm_w [head_dim] shared by all heads, then n is
// rotated, rounded and appended as above; v is untouched.  head_dim 64 or
// 128.
void launch_qk_norm_rope_kv_append(
    uint16_t* q, uint16_t* k, uint16_t* v,
    const uint16_t* q_norm_w, const uint16_t* k_norm_w, float eps,
    const int32_t* positions, const float* cos_sin,
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

// The fused decode kernel with the q/k RMSNorm of
// launch_qk_norm_rope_kv_append applied in registers before the rotation.
// block_size must be 16 (other sizes launch nothing: the caller validates).
void launch_decode_attn_fused_qknorm(
    const uint16_t* qkv, const uint16_t* q_norm_w, const uint16_t* k_norm_w,
    float eps, void* k_cache, void* v_cache,
    const int32_t* block_table, const int32_t* seq_lens,
    const int32_t* positions, const float* cos_sin,
    const int32_t* slot_mapping, uint16_t* out, int batch, int n_q_heads,
    int n_kv_heads, int head_dim, int block_size, int max_blocks,
    float scale, int qkv_stride, int n_split, float* part_out,
    float* part_ml, bool cache_fp8, hipStream_t stream);

// Shared-prefix decode attention (decode_attn_shared.hip): rows that share
// a leading run of physical KV blocks read it once per group (MFMA prefix
// phase into f32 partials), then every row walks its private blocks and
// folds its partials in.  bf16 cache, block size 16, head_dim 128, GQA
// group 4 or 8; q is read from the fused qkv rows.
//   n_shared[batch]      shared tokens of the row (a multiple of 16; 0 =
//                        in no group: a complete attention, no split-K)
//   row_tile / row_slot  the row's tile and member slot (unused at 0)
//   tile_rows[T, 64/G]   member batch rows of a tile, -1 padded
//   tile_blocks[T]       shared blocks of the tile's group
//   tile_bt_row[T]       a member row whose block table lists them
//   ws_acc / ws_ml       [T, n_kv, n_chunks, 64, head_dim] / [.., 64, 2]
// shared_prefix_n_chunks: the chunk count that fills the device, for
// `tiles` row tiles whose longest prefix spans kv_tiles 64-token tiles.
int shared_prefix_n_chunks(int tiles, int n_kv_heads, int kv_tiles);
void launch_decode_attn_shared(
    const uint16_t* qkv, const uint16_t* k_cache, const uint16_t* v_cache,
    const int32_t* block_table, const int32_t* seq_lens,
    const int32_t* n_shared, const int32_t* row_tile,
    const int32_t* row_slot, const int32_t* tile_rows,
    const int32_t* tile_blocks, const int32_t* tile_bt_row, float* ws_acc,
    float* ws_ml, uint16_t* out, int batch, int n_tiles, int n_chunks,
    int n_q_heads, int n_kv_heads, int max_blocks, float scale,
    int qkv_stride, hipStream_t stream);

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
// Zero-point forms (w4a16_zp.hip): w = f32(s) * (u - z) with u the packed
// nibble and meta[N, K/128] = fp16 s | bf16(-(128 + z)) << 16.  Same
// contract and slicing as above.
//   launch_awq_repack: AutoAWQ GEMM tensors (qweight [K, N/8], qzeros
//     [K/128, N/8], scales fp16 [K/128, N]) -> columns col_offset ..
//     col_offset + N of packed / meta; N % 64 == 0, col_offset % 64 == 0.
void launch_w4a16_zp(const uint16_t* x, const uint32_t* packed,
                     const uint32_t* meta, float* ws, uint16_t* out, int M,
                     int N, int K, int splitk, int grp_per_slice,
                     hipStream_t stream);
void launch_w4_zp_dequant(const uint32_t* packed, const uint32_t* meta,
                          uint16_t* out, int N, int K, hipStream_t stream);
void launch_awq_repack(const uint32_t* qweight, const uint32_t* qzeros,
                       const uint16_t* scales, uint32_t* packed,
                       uint32_t* meta, int N, int K, int col_offset,
                       hipStream_t stream);
// SwiGLU-fused forms (w4a16_silu.hip): launch_w4a16 / launch_w4a16_zp with
// gu [M, 2K] (packed gate|up rows) in place of x and the A fragment built
// as bf16(silu(g) * u), the rounding launch_silu_mul stores: bit-identical
// to that launch followed by the plain one, same slicing and slab.
void launch_w4a16_silu(const uint16_t* gu, const uint32_t* packed,
                       const uint16_t* s, float* ws, uint16_t* out, int M,
                       int N, int K, int splitk, int grp_per_slice,
                       hipStream_t stream);
void launch_w4a16_zp_silu(const uint16_t* gu, const uint32_t* packed,
                          const uint32_t* meta, float* ws, uint16_t* out,
                          int M, int N, int K, int splitk, int grp_per_slice,
                          hipStream_t stream);
// Tiled forms (w4a16_tiled.hip): the same contract and tensors for
// 1 <= M <= 256, one workgroup of ceil(M / 64) waves per 64-column panel x
// K-slice with the packed weight staged once through LDS.
// w4a16_tiled_plan is their slicing (whole groups, a function of N and K
// only, no empty slice); ws is the [splitk, M, N] f32 slab when splitk > 1.
void w4a16_tiled_plan(int N, int K, int splitk_req, int* splitk,
                      int* grp_per_slice);
void launch_w4a16_tiled(const uint16_t* x, const uint32_t* packed,
                        const uint16_t* s, float* ws, uint16_t* out, int M,
                        int N, int K, int splitk, int grp_per_slice,
                        hipStream_t stream);
void launch_w4a16_zp_tiled(const uint16_t* x, const uint32_t* packed,
                           const uint32_t* meta, float* ws, uint16_t* out,
                           int M, int N, int K, int splitk, int grp_per_slice,
                           hipStream_t stream);
// Wide forms (w4a16_wide.hip): the same contract and tensors for
// 1 <= M <= 512 and N % 128 == 0, one workgroup of four waves per
// 128-column panel x 128-row block x K-slice, the weight converted to bf16
// once per workgroup on its way into LDS.  w4a16_wide_plan is their
// slicing (whole groups, a function of N and K only, no empty slice); ws
// is the [splitk, M, N] f32 slab when splitk > 1.
void w4a16_wide_plan(int N, int K, int splitk_req, int* splitk,
                     int* grp_per_slice);
void launch_w4a16_wide(const uint16_t* x, const uint32_t* packed,
                       const uint16_t* s, float* ws, uint16_t* out, int M,
                       int N, int K, int splitk, int grp_per_slice,
                       hipStream_t stream);
void launch_w4a16_zp_wide(const uint16_t* x, const uint32_t* packed,
                          const uint32_t* meta, float* ws, uint16_t* out,
                          int M, int N, int K, int splitk, int grp_per_slice,
                          hipStream_t stream);

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

// sample_constrained plus nucleus (top_p) filtering and presence/frequency
// penalties: z = float(logit) - (presence + frequency * c) [c > 0] + bias,
// c counted from the row's slot of a device-resident token history; the
// top_k / min_p floor on z, then keep a survivor iff the softmax(z/T)
// mass of the survivors strictly above it is < top_p * their total (ties
// at the cut stay; top_p <= 0 or >= 1: off).  hist_slot[r] == -1: no
// history.  With `append` the chosen token is stored at the end of the
// row's slot (slots of one launch are distinct).  The logits are only
// read; no workspace (sampling_nucleus.hip).
int sample_nucleus_max_history();
void launch_sample_nucleus(
    const uint16_t* logits,            // [batch, vocab] bf16
    const int32_t* rows,               // [n_rows] row indices into logits
    const float* temperatures,         // [batch]
    const uint64_t* seeds,             // [batch]
    uint64_t step,
    const int32_t* top_k,              // [n_rows]
    const float* min_p,                // [n_rows]
    const float* top_p,                // [n_rows]
    const float* presence,             // [n_rows]
    const float* frequency,            // [n_rows]
    const int32_t* bias_offsets,       // [n_rows + 1]
    const int32_t* bias_ids,           // [n_bias_total]
    const float* bias_vals,            // [n_bias_total]
    int n_bias_total,
    const int32_t* hist_slot,          // [n_rows], -1 or a slot
    int32_t* history,                  // [n_slots, cap]
    int32_t* hist_len,                 // [n_slots]
    int n_slots, int cap, bool append,
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

// Mixture-of-Experts MLP (moe.hip).
//   launch_moe_route: ids[T, k] = the k largest logits of each row of
//     logits[T, E] bf16 (descending, ties to the lower index, NaN lowest),
//     w[T, k] = f32 softmax over all E at those ids, divided by their sum
//     with renorm.  2 <= E <= 256, 1 <= k <= min(E, 8).
//   launch_moe_mlp: out[t] = bf16(sum_j w[t, j] * down_e(bf16(silu(gate_e
//     (x[t])) * up_e(x[t])))), e = ids[t, j], w_gate_up [E, 2I, H] (gate |
//     up rows), w_down [E, H, I]; H % 64 == 0, I % 64 == 0.  Four launches
//     (align, gate/up + SwiGLU, down, combine), no host sync, no float
//     atomics.  R = moe_row_tile(T, k, E) (16 or 64) rows per tile; with
//     n = moe_max_tiles(T, k, E, R) the workspaces are sorted int32 [n * R],
//     tile_expert int32 [n], pos int32 [T * k], n_live int32 [1], act bf16
//     [n * R, I] and y f32 [n * R, H]; none needs initialising.  An id
//     outside [0, E) contributes nothing.
int moe_row_tile(int T, int k, int E);
int moe_max_tiles(int T, int k, int E, int R);
void launch_moe_route(const uint16_t* logits, int32_t* ids, float* w, int T,
                      int E, int k, bool renorm, hipStream_t stream);
void launch_moe_mlp(const uint16_t* x, const int32_t* ids, const float* w,
                    const uint16_t* w_gate_up, const uint16_t* w_down,
                    int32_t* sorted, int32_t* tile_expert, int32_t* pos,
                    int32_t* n_live, uint16_t* act, float* y, uint16_t* out,
                    int T, int k, int E, int H, int I, int R,
                    hipStream_t stream);

}  // namespace rlli
