// Fused on-device sampling over the vocab dimension.
//
// Greedy (temperature == 0): argmax of the logits row.
// Temperature sampling: Gumbel-max — argmax of logits/T + g where
// g = -log(-log(u)) — which samples softmax(logits/T) EXACTLY, in one
// reduction pass, with no 128k-wide softmax materialization and no
// host round-trip.  u comes from a counter-based hash of
// (seed, row, column): reproducible given the seed and free of the
// 32 MB/step random-tensor traffic a torch-side sampler would need.
// One workgroup per row (Llama vocab 128256 -> 256 threads x ~63 bf16x8
// vectors each); ties break to the lowest index for determinism.
// Rows with logit_bias / top_k / min_p are redrawn by
// sample_constrained_kernel (below) with the same per-element score.

#include "common.h"

namespace rlli {

namespace {

DEV_INLINE uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

DEV_INLINE float uniform01(uint64_t seed, uint64_t counter) {
  const uint64_t h = splitmix64(seed ^ splitmix64(counter));
  // 24 mantissa-ish bits -> (0, 1]; never exactly 0 so log() is finite
  return (float((h >> 40) & 0xffffffu) + 1.0f) * (1.0f / 16777217.0f);
}

struct BestPair {
  float val;
  int idx;
};

DEV_INLINE BestPair better(BestPair a, BestPair b) {
  if (b.val > a.val || (b.val == a.val && b.idx < a.idx)) return b;
  return a;
}

// The per-element score every sampler scan maximizes: the logit itself
// for greedy rows (inv_t == 1), else logit/T plus the Gumbel noise of
// (seed, idx).  One definition, so every kernel below picks the same
// token for the same (value, seed, index).
DEV_INLINE float sample_score(float z, float inv_t, bool greedy,
                              uint64_t seed, int idx) {
  float val = z * inv_t;
  if (!greedy) {
    const float u = uniform01(seed, uint64_t(idx));
    val += -__logf(-__logf(u));
  }
  return val;
}

__global__ __launch_bounds__(256)
void sample_kernel(const uint16_t* __restrict__ logits,
                   const float* __restrict__ temperatures,
                   const uint64_t* __restrict__ seeds, uint64_t step,
                   int32_t* __restrict__ out_tokens, int vocab) {
  const int row = blockIdx.x;
  const float temp = temperatures[row];
  const bool greedy = temp <= 0.f;
  const float inv_t = greedy ? 1.f : 1.f / temp;
  // per-request reproducibility: the row's seed (client-provided or
  // engine default) mixed with the per-sequence step counter in-kernel,
  // so the decode pipeline never uploads per-step randomness
  const uint64_t seed = splitmix64(seeds[row] + 0x9e3779b97f4a7c15ull * step);

  BestPair best{-1e30f, 0};
  const int nvec = vocab / 8;
  const int stride = blockDim.x;
  int v8 = threadIdx.x;
  // 4 row-vectors in flight per lane before any arithmetic (one
  // outstanding load per lane left this walk latency-bound); `better`
  // is associative with a lowest-index tie-break, so the reordering
  // cannot change the sampled token
  for (; v8 + 3 * stride < nvec; v8 += 4 * stride) {
    uint4 raw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      raw[j] = *reinterpret_cast<const uint4*>(
          logits + int64_t(row) * vocab + (v8 + j * stride) * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x8 lv;
      lv.u = raw[j];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int idx = (v8 + j * stride) * 8 + i;
        const float val =
            sample_score(bf16_to_f32(lv.s[i]), inv_t, greedy, seed, idx);
        best = better(best, BestPair{val, idx});
      }
    }
  }
  for (; v8 < nvec; v8 += stride) {
    bf16x8 lv;
    lv.u = *reinterpret_cast<const uint4*>(logits + int64_t(row) * vocab + v8 * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = v8 * 8 + i;
      const float val =
          sample_score(bf16_to_f32(lv.s[i]), inv_t, greedy, seed, idx);
      best = better(best, BestPair{val, idx});
    }
  }
  // vocab tail (vocab % 8)
  for (int idx = nvec * 8 + threadIdx.x; idx < vocab; idx += blockDim.x) {
    const float val =
        sample_score(bf16_to_f32(logits[int64_t(row) * vocab + idx]), inv_t,
                     greedy, seed, idx);
    best = better(best, BestPair{val, idx});
  }

  // wave reduction of (val, idx)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    BestPair other{__shfl_xor(best.val, off, kWave),
                   __shfl_xor(best.idx, off, kWave)};
    best = better(best, other);
  }
  __shared__ float lds_val[4];
  __shared__ int lds_idx[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_val[wave] = best.val;
    lds_idx[wave] = best.idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    BestPair final_best{lds_val[0], lds_idx[0]};
    const int n_waves = blockDim.x >> 6;
    for (int w = 1; w < n_waves; ++w)
      final_best = better(final_best, BestPair{lds_val[w], lds_idx[w]});
    out_tokens[row] = final_best.idx;
  }
}

// ---- two-phase split-row variant ----
// One WG per row leaves 64 WGs on 256 CUs at decode batch 64 (quarter
// fill): greedy measured 20.4 us and gumbel 92.6 us isolated.  Phase A
// gives each of n_split WGs a contiguous vocab chunk and packs its local
// (val, idx) into one orderable uint64 (val bits flipped sign-magnitude
// -> monotone unsigned; low word 0x7fffffff-idx so equal values prefer
// the LOWEST index, matching better()); phase B is one tiny reduction.
// Token selection is bit-identical to the single-phase kernel: the same
// per-(seed, idx) value is computed for every index, only the scan
// partitioning changes.

DEV_INLINE uint64_t pack_best(BestPair b) {
  uint32_t u = __float_as_uint(b.val);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (uint64_t(u) << 32) | uint32_t(0x7fffffff - b.idx);
}

__global__ __launch_bounds__(256)
void sample_part_kernel(const uint16_t* __restrict__ logits,
                        const float* __restrict__ temperatures,
                        const uint64_t* __restrict__ seeds, uint64_t step,
                        uint64_t* __restrict__ partials, int vocab,
                        int n_split) {
  const int row = blockIdx.x;
  const int split = blockIdx.y;
  const float temp = temperatures[row];
  const bool greedy = temp <= 0.f;
  const float inv_t = greedy ? 1.f : 1.f / temp;
  const uint64_t seed = splitmix64(seeds[row] + 0x9e3779b97f4a7c15ull * step);

  const int nvec = vocab / 8;
  const int chunk = (nvec + n_split - 1) / n_split;
  const int v0 = split * chunk;
  const int v1 = min(nvec, v0 + chunk);
  const uint16_t* lrow = logits + int64_t(row) * vocab;

  BestPair best{-1e30f, 0};
  const int stride = blockDim.x;
  int v8 = v0 + threadIdx.x;
  for (; v8 + 3 * stride < v1; v8 += 4 * stride) {
    uint4 raw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      raw[j] = *reinterpret_cast<const uint4*>(lrow + (v8 + j * stride) * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x8 lv;
      lv.u = raw[j];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int idx = (v8 + j * stride) * 8 + i;
        const float val =
            sample_score(bf16_to_f32(lv.s[i]), inv_t, greedy, seed, idx);
        best = better(best, BestPair{val, idx});
      }
    }
  }
  for (; v8 < v1; v8 += stride) {
    bf16x8 lv;
    lv.u = *reinterpret_cast<const uint4*>(lrow + v8 * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = v8 * 8 + i;
      const float val =
          sample_score(bf16_to_f32(lv.s[i]), inv_t, greedy, seed, idx);
      best = better(best, BestPair{val, idx});
    }
  }
  if (split == n_split - 1) {                  // vocab % 8 tail
    for (int idx = nvec * 8 + threadIdx.x; idx < vocab; idx += blockDim.x) {
      const float val =
          sample_score(bf16_to_f32(lrow[idx]), inv_t, greedy, seed, idx);
      best = better(best, BestPair{val, idx});
    }
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    BestPair other{__shfl_xor(best.val, off, kWave),
                   __shfl_xor(best.idx, off, kWave)};
    best = better(best, other);
  }
  __shared__ float lds_val[4];
  __shared__ int lds_idx[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_val[wave] = best.val;
    lds_idx[wave] = best.idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    BestPair fb{lds_val[0], lds_idx[0]};
    const int n_waves = blockDim.x >> 6;
    for (int w = 1; w < n_waves; ++w)
      fb = better(fb, BestPair{lds_val[w], lds_idx[w]});
    partials[int64_t(row) * n_split + split] = pack_best(fb);
  }
}

__global__ __launch_bounds__(64)
void sample_final_kernel(const uint64_t* __restrict__ partials,
                         int32_t* __restrict__ out_tokens, int rows,
                         int n_split) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  uint64_t best = 0;
  for (int s = 0; s < n_split; ++s)
    best = max(best, partials[int64_t(row) * n_split + s]);
  out_tokens[row] = 0x7fffffff - int(best & 0xffffffffu);
}

// ---- constrained rows: logit_bias, top_k, min_p ----
// One 1024-thread workgroup per SELECTED row (such rows are few, and a
// row is L2-resident right after the lm_head GEMM, so it is simply
// walked once per pass).  With z = float(x) + bias (f32, rounded once):
//   pass 1      z_max, and the histogram of the top 11 bits of key(z)
//   pass 2, 3   the remaining 11 + 10 key bits of the k-th largest z
//               (radix select; key = pack_best's monotone u32 image)
//   last pass   Gumbel arg-max of sample_score over z >= max(thr_k, thr_p)
// with thr_k the k-th largest z (boundary ties all stay) and
// thr_p = z_max + T*ln(min_p).  Greedy rows and rows with both filters
// off run only the last pass.  The bias is found through a one-bit-per-
// token LDS bitmap (one byte per bf16x8 vector); only a hit searches the
// row's ascending id list.  Histograms are LDS integer adds and nothing
// goes through global atomics: repeated calls are bit-identical.  The
// logits are only read.

constexpr int kCsThreads = 1024;
constexpr int kCsWaves = kCsThreads / kWave;
constexpr int kCsMaxVocab = 262144;              // bitmap: 32 KB of LDS
constexpr int kCsBins = 2048;                    // 11-bit radix digit

DEV_INLINE uint32_t mono32(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEV_INLINE float mono32_to_f32(uint32_t m) {
  return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

// 8 bf16 at p, which is only as aligned as `mis` (= address & 15 of the
// row base; every vector offset is a multiple of 16 B) says
DEV_INLINE uint4 load_vec8(const uint16_t* p, uint32_t mis) {
  if (mis == 0) return *reinterpret_cast<const uint4*>(p);
  if ((mis & 7u) == 0) {
    const uint2 a = *reinterpret_cast<const uint2*>(p);
    const uint2 b = *reinterpret_cast<const uint2*>(p + 4);
    return make_uint4(a.x, a.y, b.x, b.y);
  }
  if ((mis & 3u) == 0) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    return make_uint4(q[0], q[1], q[2], q[3]);
  }
  return make_uint4(p[0] | uint32_t(p[1]) << 16, p[2] | uint32_t(p[3]) << 16,
                    p[4] | uint32_t(p[5]) << 16, p[6] | uint32_t(p[7]) << 16);
}

// bias of token idx, known to be in ids[0, n) (ascending)
DEV_INLINE float find_bias(const int32_t* __restrict__ ids,
                           const float* __restrict__ vals, int n, int idx) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < idx) lo = mid + 1; else hi = mid;
  }
  return ids[lo] == idx ? vals[lo] : 0.f;
}

// f(z, idx) for every token of the row this thread owns; two vectors in
// flight per lane before any arithmetic
template <typename F>
DEV_INLINE void scan_biased_row(const uint16_t* __restrict__ lrow, int vocab,
                                uint32_t mis, const uint32_t* bitmap,
                                const int32_t* __restrict__ ids,
                                const float* __restrict__ vals, int n_bias,
                                F&& f) {
  const int nvec = vocab / 8;
  auto one_vec = [&](uint4 raw, int v) {
    bf16x8 lv;
    lv.u = raw;
    const uint32_t hit =
        n_bias > 0 ? (bitmap[v >> 2] >> ((v & 3) * 8)) & 0xffu : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float z = bf16_to_f32(lv.s[i]);
      if (hit >> i & 1u) z += find_bias(ids, vals, n_bias, v * 8 + i);
      f(z, v * 8 + i);
    }
  };
  int v = threadIdx.x;
  for (; v + kCsThreads < nvec; v += 2 * kCsThreads) {
    const uint4 r0 = load_vec8(lrow + v * 8, mis);
    const uint4 r1 = load_vec8(lrow + (v + kCsThreads) * 8, mis);
    one_vec(r0, v);
    one_vec(r1, v + kCsThreads);
  }
  for (; v < nvec; v += kCsThreads) one_vec(load_vec8(lrow + v * 8, mis), v);
  for (int idx = nvec * 8 + threadIdx.x; idx < vocab; idx += kCsThreads) {
    float z = bf16_to_f32(lrow[idx]);
    if (n_bias > 0 && (bitmap[idx >> 5] >> (idx & 31) & 1u))
      z += find_bias(ids, vals, n_bias, idx);
    f(z, idx);
  }
}

// Wave 0: the highest bin at which the count from the top reaches *need.
// Lane l sums the l-th group of bins from the top; the lane whose group
// crosses walks it.  Leaves the bin in *sel and what is still needed
// inside it in *need.
DEV_INLINE void select_bin(const uint32_t* hist, int n_bins, uint32_t* sel,
                           uint32_t* need) {
  const int lane = threadIdx.x;
  const int per = n_bins / kWave;
  const int top = n_bins - 1 - lane * per;       // this lane's highest bin
  uint32_t own = 0;
  // rotated start: lanes' bins are `per` words apart, which would put
  // them all in one bank
  for (int i = 0; i < per; ++i) own += hist[top - ((i + lane) & (per - 1))];
  uint32_t incl = own;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t o = uint32_t(__shfl_up(int(incl), off, kWave));
    if (lane >= off) incl += o;
  }
  const uint32_t k = *need;
  const uint64_t crossed = __ballot(incl >= k);
  if (crossed != 0 && lane == __ffsll((long long)crossed) - 1) {
    uint32_t above = incl - own;
    int b = top;
    for (int i = 0; i < per - 1 && above + hist[b] < k; ++i, --b)
      above += hist[b];
    *sel = uint32_t(b);
    *need = k - above;
  }
}

__global__ __launch_bounds__(kCsThreads)
void sample_constrained_kernel(const uint16_t* __restrict__ logits,
                               const int32_t* __restrict__ rows,
                               const float* __restrict__ temperatures,
                               const uint64_t* __restrict__ seeds,
                               uint64_t step,
                               const int32_t* __restrict__ top_k,
                               const float* __restrict__ min_p,
                               const int32_t* __restrict__ bias_offsets,
                               const int32_t* __restrict__ bias_ids,
                               const float* __restrict__ bias_vals,
                               int n_bias_total,
                               int32_t* __restrict__ out_tokens, int vocab) {
  __shared__ uint32_t bitmap[kCsMaxVocab / 32];
  __shared__ uint32_t hist[kCsBins];
  __shared__ float red_val[kCsWaves];
  __shared__ int red_idx[kCsWaves];
  __shared__ uint32_t sel_bin, sel_need;

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int row = rows[r];
  const float temp = temperatures[row];
  const bool greedy = temp <= 0.f;
  const float inv_t = greedy ? 1.f : 1.f / temp;
  const uint64_t seed = splitmix64(seeds[row] + 0x9e3779b97f4a7c15ull * step);
  const uint16_t* lrow = logits + int64_t(row) * vocab;
  const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(lrow)) & 15u;

  // the row's slice of the CSR bias list, clamped into the arrays
  const int b0 = min(max(bias_offsets[r], 0), n_bias_total);
  const int b1 = min(max(bias_offsets[r + 1], b0), n_bias_total);
  const int n_bias = b1 - b0;
  const int32_t* ids = bias_ids + b0;
  const float* vals = bias_vals + b0;
  if (n_bias > 0) {
    for (int i = tid; i < (vocab + 31) / 32; i += kCsThreads) bitmap[i] = 0u;
    __syncthreads();
    for (int i = tid; i < n_bias; i += kCsThreads) {
      const int id = ids[i];
      if (id >= 0 && id < vocab) atomicOr(&bitmap[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }
  auto scan = [&](auto&& f) {
    scan_biased_row(lrow, vocab, mis, bitmap, ids, vals, n_bias, f);
  };

  const int k = top_k[r];
  const float mp = min_p[r];
  const bool use_k = !greedy && k >= 1 && k < vocab;
  const bool use_p = !greedy && mp > 0.f;
  float thr = -INFINITY;
  if (use_k || use_p) {
    if (use_k) {
      for (int i = tid; i < kCsBins; i += kCsThreads) hist[i] = 0u;
      if (tid == 0) sel_need = uint32_t(k);
      __syncthreads();
    }
    float zmax = -INFINITY;
    scan([&](float z, int) {
      zmax = fmaxf(zmax, z);
      if (use_k) atomicAdd(&hist[mono32(z) >> 21], 1u);
    });
    zmax = wave_max(zmax);
    if ((tid & 63) == 0) red_val[tid >> 6] = zmax;
    __syncthreads();
    zmax = red_val[0];
#pragma unroll
    for (int w = 1; w < kCsWaves; ++w) zmax = fmaxf(zmax, red_val[w]);
    if (use_p) thr = zmax + temp * logf(mp);
    if (use_k) {
      // digits of the k-th largest key, most significant first
      if (tid < kWave) select_bin(hist, kCsBins, &sel_bin, &sel_need);
      __syncthreads();
      uint32_t prefix = sel_bin;                    // key >> 21
      for (int i = tid; i < kCsBins; i += kCsThreads) hist[i] = 0u;
      __syncthreads();
      scan([&](float z, int) {
        const uint32_t key = mono32(z);
        if (key >> 21 == prefix) atomicAdd(&hist[key >> 10 & 2047u], 1u);
      });
      __syncthreads();
      if (tid < kWave) select_bin(hist, kCsBins, &sel_bin, &sel_need);
      __syncthreads();
      prefix = prefix << 11 | sel_bin;              // key >> 10
      for (int i = tid; i < 1024; i += kCsThreads) hist[i] = 0u;
      __syncthreads();
      scan([&](float z, int) {
        const uint32_t key = mono32(z);
        if (key >> 10 == prefix) atomicAdd(&hist[key & 1023u], 1u);
      });
      __syncthreads();
      if (tid < kWave) select_bin(hist, 1024, &sel_bin, &sel_need);
      __syncthreads();
      thr = fmaxf(thr, mono32_to_f32(prefix << 10 | sel_bin));
    }
    __syncthreads();                                // red_val is reused below
  }

  BestPair best{-1e30f, 0};
  scan([&](float z, int idx) {
    if (z >= thr)
      best = better(best,
                    BestPair{sample_score(z, inv_t, greedy, seed, idx), idx});
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    BestPair other{__shfl_xor(best.val, off, kWave),
                   __shfl_xor(best.idx, off, kWave)};
    best = better(best, other);
  }
  if ((tid & 63) == 0) {
    red_val[tid >> 6] = best.val;
    red_idx[tid >> 6] = best.idx;
  }
  __syncthreads();
  if (tid == 0) {
    BestPair fb{red_val[0], red_idx[0]};
    for (int w = 1; w < kCsWaves; ++w)
      fb = better(fb, BestPair{red_val[w], red_idx[w]});
    out_tokens[r] = fb.idx;
  }
}

}  // namespace

int sample_n_split(int batch) {
  // fill 256 CUs: >=512 WGs when possible, capped so chunks stay >=4096
  // logits (16 splits at vocab 128k)
  if (batch <= 0) return 1;   // chunk-only mixed steps sample 0 rows
  int n = (512 + batch - 1) / batch;
  if (n > 16) n = 16;
  if (n < 1) n = 1;
  return n;
}

void launch_sample(const uint16_t* logits, const float* temperatures,
                   const uint64_t* seeds, uint64_t step, int32_t* out_tokens,
                   int batch, int vocab, uint64_t* partials, int n_split,
                   hipStream_t stream) {
  if (batch == 0) return;
  if (n_split <= 1 || partials == nullptr) {
    hipLaunchKernelGGL(sample_kernel, dim3(batch), dim3(256), 0, stream,
                       logits, temperatures, seeds, step, out_tokens, vocab);
    return;
  }
  hipLaunchKernelGGL(sample_part_kernel, dim3(batch, n_split), dim3(256), 0,
                     stream, logits, temperatures, seeds, step, partials,
                     vocab, n_split);
  hipLaunchKernelGGL(sample_final_kernel, dim3((batch + 63) / 64), dim3(64),
                     0, stream, partials, out_tokens, batch, n_split);
}

int sample_constrained_max_vocab() { return kCsMaxVocab; }

void launch_sample_constrained(const uint16_t* logits, const int32_t* rows,
                               const float* temperatures,
                               const uint64_t* seeds, uint64_t step,
                               const int32_t* top_k, const float* min_p,
                               const int32_t* bias_offsets,
                               const int32_t* bias_ids,
                               const float* bias_vals, int n_bias_total,
                               int32_t* out_tokens, int n_rows, int vocab,
                               hipStream_t stream) {
  if (n_rows == 0) return;
  hipLaunchKernelGGL(sample_constrained_kernel, dim3(n_rows),
                     dim3(kCsThreads), 0, stream, logits, rows, temperatures,
                     seeds, step, top_k, min_p, bias_offsets, bias_ids,
                     bias_vals, n_bias_total, out_tokens, vocab);
}

}  // namespace rlli
