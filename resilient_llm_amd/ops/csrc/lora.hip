// Batched multi-adapter LoRA: row t of the batch uses adapter
// adapter_idx[t] (-1 = none).  The low-rank update runs NEXT TO the base
// GEMM, which is untouched:
//
//   lora_shrink       y[t, r]    = sum_k x[t, k] * A[a, r, k]          (f32)
//   lora_expand_add_  out[t, o] = bf16(float(out[t, o])
//                                 + scale[a] * sum_j y[t, s*r_max + j] * B[a, o, j])
//
// with a = adapter_idx[t] and s the slice of output row o: the fused
// projections (q|k|v, gate|up) stack one A per slice along the rank axis
// (R = n_slices * r_max, zero-padded) and output row o of slice s reads
// ranks [s*r_max, (s+1)*r_max) of the shrink result.
//
// Shrink: one wave per 4 ranks, lanes stride K as 16-byte bf16x8 vectors,
// f32 accumulation, a wave-level xor reduction, one plain store per
// (t, r) — no atomics, no split-K.  Expand: one thread per output row o,
// the tokens' y rows staged through LDS, a fixed-order fma chain over
// r_max and ONE rounding at the final add; every element has exactly one
// writer.  Rows with adapter_idx -1 (or an index outside the stack) are
// skipped before their first load in both kernels.
//
// Token tiles: a workgroup covers TPB consecutive tokens — 1 for decode-
// sized batches, where the launch needs every workgroup it can get, 4
// from 512 rows (prefill) up.  When the 4 tokens of a tile share one
// adapter, as the rows of a prompt do, A (or the B row) is loaded once
// for the four of them: without that a long prefill re-reads the whole
// A/B stack per token and sits on the L2's bandwidth.  Any other tile
// runs its tokens one after the other.  Every (t, r) and (t, o) is summed
// in the same order on every path, so results do not depend on T, on the
// tile size or on the neighbours' adapters, and repeated calls are
// bit-identical.  (Tiling decode batches too was measured and rejected:
// profiles/lora.md.)
//
// All offsets into A, B, x, y and out are 64-bit.  K, O and r_max need
// not be multiples of anything: the 16-byte loads are a template arm
// taken when the row pitch and base pointers allow it, scalar loads
// otherwise.

#include "common.h"

#include <climits>

namespace rlli {

namespace {

constexpr int THREADS = 256;
constexpr int RANKS_PER_WAVE = 4;
constexpr int RANKS_PER_BLOCK = (THREADS / kWave) * RANKS_PER_WAVE;
constexpr int MAX_SLICES = 3;
constexpr int MAX_RANK = 64;
constexpr int MAX_R = MAX_SLICES * MAX_RANK;      // 192 <= THREADS
constexpr int TILE = 4;                           // tokens per tiled block
constexpr int TILE_MIN_ROWS = 512;                // tile from this T up

// Adapters of the TPB tokens from t0 on: -1 past T or outside the stack.
// Returns whether all TPB are one valid adapter.
template <int TPB>
DEV_INLINE bool tile_adapters(const int32_t* __restrict__ adapter_idx,
                              int64_t t0, int T, int n_adapters, int* a) {
  bool uniform = true;
#pragma unroll
  for (int n = 0; n < TPB; ++n) {
    int v = (t0 + n < T) ? adapter_idx[t0 + n] : -1;
    if (v >= n_adapters) v = -1;
    a[n] = v < 0 ? -1 : v;
    uniform = uniform && a[n] >= 0 && a[n] == a[0];
  }
  return uniform;
}

// y[t0 + n, r0 .. r0+3] for n < NT tokens that all use adapter a.
template <bool VEC, int NT>
DEV_INLINE void shrink_rows(const uint16_t* __restrict__ x,
                            const uint16_t* __restrict__ A,
                            float* __restrict__ y, int64_t t0, int a, int r0,
                            int R, int K, int lane) {
  // ranks past R re-read rank R-1 (no divergent loads) and are not stored
  const uint16_t* ar[RANKS_PER_WAVE];
#pragma unroll
  for (int i = 0; i < RANKS_PER_WAVE; ++i)
    ar[i] = A + (int64_t(a) * R + min(r0 + i, R - 1)) * K;
  float acc[NT][RANKS_PER_WAVE];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int i = 0; i < RANKS_PER_WAVE; ++i) acc[n][i] = 0.f;
  if constexpr (VEC) {
    const int kv = K >> 3;
    for (int v = lane; v < kv; v += kWave) {
      bf16x8 av[RANKS_PER_WAVE];
#pragma unroll
      for (int i = 0; i < RANKS_PER_WAVE; ++i)
        av[i].u = reinterpret_cast<const uint4*>(ar[i])[v];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        bf16x8 xv;
        xv.u = reinterpret_cast<const uint4*>(x + (t0 + n) * K)[v];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xf = bf16_to_f32(xv.s[j]);
#pragma unroll
          for (int i = 0; i < RANKS_PER_WAVE; ++i)
            acc[n][i] = fmaf(xf, bf16_to_f32(av[i].s[j]), acc[n][i]);
        }
      }
    }
  } else {
    for (int k = lane; k < K; k += kWave) {
      float af[RANKS_PER_WAVE];
#pragma unroll
      for (int i = 0; i < RANKS_PER_WAVE; ++i) af[i] = bf16_to_f32(ar[i][k]);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float xf = bf16_to_f32(x[(t0 + n) * K + k]);
#pragma unroll
        for (int i = 0; i < RANKS_PER_WAVE; ++i)
          acc[n][i] = fmaf(xf, af[i], acc[n][i]);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int i = 0; i < RANKS_PER_WAVE; ++i) {
      const float sum = wave_sum(acc[n][i]);
      if (lane == 0 && r0 + i < R) y[(t0 + n) * R + r0 + i] = sum;
    }
}

template <bool VEC, int TPB>
__global__ __launch_bounds__(THREADS)
void lora_shrink_kernel(const uint16_t* __restrict__ x,
                        const uint16_t* __restrict__ A,
                        const int32_t* __restrict__ adapter_idx,
                        float* __restrict__ y, int T, int n_adapters, int R,
                        int K) {
  const int64_t t0 = int64_t(blockIdx.x) * TPB;
  int a[TPB];
  const bool uniform = tile_adapters<TPB>(adapter_idx, t0, T, n_adapters, a);
  const int lane = threadIdx.x & (kWave - 1);
  const int r0 = blockIdx.y * RANKS_PER_BLOCK
      + (threadIdx.x / kWave) * RANKS_PER_WAVE;
  if (r0 >= R) return;                            // wave-uniform
  if (TPB > 1 && uniform) {
    shrink_rows<VEC, TPB>(x, A, y, t0, a[0], r0, R, K, lane);
    return;
  }
#pragma unroll
  for (int n = 0; n < TPB; ++n)
    if (a[n] >= 0) shrink_rows<VEC, 1>(x, A, y, t0 + n, a[n], r0, R, K, lane);
}

// out[t0 + n, o] for n < NT tokens that all use adapter a; ys holds the
// tokens' y rows, MAX_R floats apart.
template <bool VEC, int NT>
DEV_INLINE void expand_rows(uint16_t* __restrict__ out, const float* ys,
                            const uint16_t* __restrict__ B,
                            const float* __restrict__ scale, int64_t t0,
                            int a, int o, int O, int r_max, int s) {
  const uint16_t* br = B + (int64_t(a) * O + o) * r_max;
  const float* yr = ys + s * r_max;
  float sum[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) sum[n] = 0.f;
  if constexpr (VEC) {
    for (int j = 0; j < r_max; j += 8) {
      bf16x8 bv;
      bv.u = *reinterpret_cast<const uint4*>(br + j);
      float bf[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) bf[e] = bf16_to_f32(bv.s[e]);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float4 y0 =
            *reinterpret_cast<const float4*>(yr + n * MAX_R + j);
        const float4 y1 =
            *reinterpret_cast<const float4*>(yr + n * MAX_R + j + 4);
        float v = sum[n];
        v = fmaf(y0.x, bf[0], v);
        v = fmaf(y0.y, bf[1], v);
        v = fmaf(y0.z, bf[2], v);
        v = fmaf(y0.w, bf[3], v);
        v = fmaf(y1.x, bf[4], v);
        v = fmaf(y1.y, bf[5], v);
        v = fmaf(y1.z, bf[6], v);
        v = fmaf(y1.w, bf[7], v);
        sum[n] = v;
      }
    }
  } else {
    for (int j = 0; j < r_max; ++j) {
      const float bf = bf16_to_f32(br[j]);
#pragma unroll
      for (int n = 0; n < NT; ++n)
        sum[n] = fmaf(yr[n * MAX_R + j], bf, sum[n]);
    }
  }
  // the contract's single rounding: an f32 product, an f32 add, one
  // conversion to bf16 (no contraction of the two into an fma)
  const float sc = scale[a];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    uint16_t* po = out + (t0 + n) * O + o;
    *po = f32_to_bf16(__fadd_rn(bf16_to_f32(*po), __fmul_rn(sc, sum[n])));
  }
}

template <bool VEC, int TPB>
__global__ __launch_bounds__(THREADS)
void lora_expand_add_kernel(uint16_t* __restrict__ out,
                            const float* __restrict__ y,
                            const uint16_t* __restrict__ B,
                            const float* __restrict__ scale,
                            const int32_t* __restrict__ adapter_idx, int T,
                            int n_adapters, int O, int r_max, int R,
                            int end0, int end1) {
  __shared__ __attribute__((aligned(16))) float ys[TPB * MAX_R];
  const int64_t t0 = int64_t(blockIdx.x) * TPB;
  int a[TPB];
  const bool uniform = tile_adapters<TPB>(adapter_idx, t0, T, n_adapters, a);
  bool any = false;
#pragma unroll
  for (int n = 0; n < TPB; ++n) {
    any = any || a[n] >= 0;
    if (a[n] >= 0 && int(threadIdx.x) < R)
      ys[n * MAX_R + threadIdx.x] = y[(t0 + n) * R + threadIdx.x];
  }
  if (!any) return;                               // block-uniform
  __syncthreads();
  const int o = blockIdx.y * THREADS + threadIdx.x;
  if (o >= O) return;
  // slice of this output row: boundaries absent from the table are INT_MAX
  const int s = int(o >= end0) + int(o >= end1);
  if (TPB > 1 && uniform) {
    expand_rows<VEC, TPB>(out, ys, B, scale, t0, a[0], o, O, r_max, s);
    return;
  }
#pragma unroll
  for (int n = 0; n < TPB; ++n)
    if (a[n] >= 0)
      expand_rows<VEC, 1>(out, ys + n * MAX_R, B, scale, t0 + n, a[n], o, O,
                          r_max, s);
}

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

}  // namespace

void launch_lora_shrink(const uint16_t* x, const uint16_t* A,
                        const int32_t* adapter_idx, float* y, int T,
                        int n_adapters, int R, int K, hipStream_t stream) {
  if (T == 0 || R == 0) return;
  const bool vec = K % 8 == 0 && aligned16(x) && aligned16(A);
  const bool tiled = T >= TILE_MIN_ROWS;
  const int tpb = tiled ? TILE : 1;
  const dim3 grid((T + tpb - 1) / tpb,
                  (R + RANKS_PER_BLOCK - 1) / RANKS_PER_BLOCK);
  auto kernel = vec ? (tiled ? lora_shrink_kernel<true, TILE>
                             : lora_shrink_kernel<true, 1>)
                    : (tiled ? lora_shrink_kernel<false, TILE>
                             : lora_shrink_kernel<false, 1>);
  hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, stream, x, A,
                     adapter_idx, y, T, n_adapters, R, K);
}

void launch_lora_expand_add(uint16_t* out, const float* y, const uint16_t* B,
                            const float* scale, const int32_t* adapter_idx,
                            int T, int n_adapters, int O, int r_max,
                            int n_slices, const int* slice_ends,
                            hipStream_t stream) {
  if (T == 0 || O == 0) return;
  const int R = n_slices * r_max;
  // row o is in slice (o >= ends[0]) + (o >= ends[1]); the last end is O
  const int end0 = n_slices > 1 ? slice_ends[0] : INT_MAX;
  const int end1 = n_slices > 2 ? slice_ends[1] : INT_MAX;
  const bool vec = r_max % 8 == 0 && aligned16(B);
  const bool tiled = T >= TILE_MIN_ROWS;
  const int tpb = tiled ? TILE : 1;
  const dim3 grid((T + tpb - 1) / tpb, (O + THREADS - 1) / THREADS);
  auto kernel = vec ? (tiled ? lora_expand_add_kernel<true, TILE>
                             : lora_expand_add_kernel<true, 1>)
                    : (tiled ? lora_expand_add_kernel<false, TILE>
                             : lora_expand_add_kernel<false, 1>);
  hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, stream, out, y, B, scale,
                     adapter_idx, T, n_adapters, O, r_max, R, end0, end1);
}

}  // namespace rlli
