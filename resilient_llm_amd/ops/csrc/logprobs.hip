// Fused log-probabilities of emitted tokens + top-k alternatives over the
// vocab dimension (OpenAI `logprobs` / `top_logprobs`).
//
//   lp(r, j) = x[j] - (m + log(sum_j exp(x[j] - m)))
//
// x is the row's RAW bf16 logits widened to f32 and m the row max: the
// numbers describe the model's distribution, independent of temperature,
// top-p and penalties (those shape which token is drawn, not what the
// model believed).  A torch composition (log_softmax + topk + gather)
// materializes a [B, V] f32 copy per step; here every logit is read from
// memory once and nothing vocab-wide is written.
//
// Same two-phase split-row shape as the sampler (sampling.hip):
//  phase A  grid (R, n_split) x 256 threads: each workgroup owns one
//           contiguous chunk (<= 8192 logits) of one selected row, held
//           ENTIRELY IN REGISTERS as 32 orderable 32-bit keys per thread
//           (bf16 bits flipped to a monotone u16 | 0xffff - local index).
//           It writes the chunk's (max, sumexp) and its k largest keys.
//  phase B  one wave per row: merges the (max, sumexp) pairs, reduces the
//           n_split*k candidates to k, and reads logits[row, token].
// Candidates travel as the sampler's pack_best key (value bits flipped to
// a monotone u32, low word 0x7fffffff - index): keys are distinct, so
// "the k largest keys" is the whole specification — value descending,
// index ascending on ties — and round j is simply max{key < winner j-1}.
// No atomics anywhere: repeated calls are bit-identical.

#include "common.h"
#include "kernels.h"

namespace rlli {

namespace {

constexpr int kLpThreads = 256;
constexpr int kLpVecs = 4;                          // bf16x8 vectors per thread
constexpr int kLpKeys = kLpVecs * 8;                // keys per thread
constexpr int kLpChunkMax = kLpThreads * kLpKeys;   // 8192 logits per workgroup
constexpr int kLpCandRegs = 8;                      // phase B candidates per lane

// bf16 bits -> u16 whose unsigned order is the float order (-0 folded
// into +0 so equal VALUES get equal keys); never 0 for a non-NaN input
DEV_INLINE uint32_t mono16(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

DEV_INLINE float mono16_to_f32(uint32_t m) {
  const uint32_t b = (m & 0x8000u) ? (m ^ 0x8000u) : (~m & 0xffffu);
  return __uint_as_float(b << 16);
}

// chunk-local key: larger = better value, ties prefer the LOWER index;
// 0 is reserved for "no element" (slot past the chunk end / removed)
DEV_INLINE uint32_t make_key(uint32_t bf16_bits, int local) {
  return (mono16(bf16_bits) << 16) | uint32_t(0xffff - local);
}

// chunk-local key -> the sampler's pack_best layout with a row-global index
DEV_INLINE uint64_t widen_key(uint32_t key, int e0) {
  const uint32_t f = __float_as_uint(mono16_to_f32(key >> 16));
  const uint32_t u = (f & 0x80000000u) ? ~f : (f | 0x80000000u);
  const int idx = e0 + int(0xffffu - (key & 0xffffu));
  return (uint64_t(u) << 32) | uint32_t(0x7fffffff - idx);
}

DEV_INLINE float key64_value(uint64_t key) {
  const uint32_t u = uint32_t(key >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

DEV_INLINE uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = max(v, uint32_t(__shfl_xor(int(v), off, kWave)));
  return v;
}

DEV_INLINE uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(v)), off, kWave));
    const uint32_t hi = uint32_t(__shfl_xor(int(uint32_t(v >> 32)), off, kWave));
    v = max(v, (uint64_t(hi) << 32) | lo);
  }
  return v;
}

__global__ __launch_bounds__(kLpThreads)
void logprobs_part_kernel(const uint16_t* __restrict__ logits,
                          const int32_t* __restrict__ rows,
                          float* __restrict__ stats,
                          uint64_t* __restrict__ cand, int vocab, int n_split,
                          int chunk, int k) {
  const int r = blockIdx.x;
  const int split = blockIdx.y;
  const int tid = threadIdx.x;
  const int e0 = split * chunk;
  const int n = min(vocab, e0 + chunk) - e0;      // <= 0: empty chunk
  const uint16_t* src = logits + int64_t(rows[r]) * vocab + e0;
  // row bases are only 2-byte aligned when vocab % 8 != 0.  e0 and every
  // vector offset are multiples of 8 elements (16 B), so the chunk's
  // first address decides for all its vectors: 16-, 8-, 4- or 2-byte
  // loads, the widest the address allows (workgroup-uniform branch)
  const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(src)) & 15u;

  // all full vectors' loads in flight before any arithmetic (as the
  // sampler); bf16x8 element i sits in bits 16*(i%2) of dword i/2
  uint4 raw[kLpVecs];
#pragma unroll
  for (int j = 0; j < kLpVecs; ++j) {
    const int off = (j * kLpThreads + tid) * 8;
    raw[j] = make_uint4(0, 0, 0, 0);
    if (off + 8 > n) continue;
    const uint16_t* p = src + off;
    if (mis == 0) {
      raw[j] = *reinterpret_cast<const uint4*>(p);
    } else if ((mis & 7u) == 0) {
      const uint2 a = *reinterpret_cast<const uint2*>(p);
      const uint2 b = *reinterpret_cast<const uint2*>(p + 4);
      raw[j] = make_uint4(a.x, a.y, b.x, b.y);
    } else if ((mis & 3u) == 0) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
      raw[j] = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
      raw[j] = make_uint4(p[0] | uint32_t(p[1]) << 16,
                          p[2] | uint32_t(p[3]) << 16,
                          p[4] | uint32_t(p[5]) << 16,
                          p[6] | uint32_t(p[7]) << 16);
    }
  }
  uint32_t key[kLpKeys];
#pragma unroll
  for (int j = 0; j < kLpVecs; ++j) {
    const int off = (j * kLpThreads + tid) * 8;
    if (off + 8 <= n) {
      bf16x8 lv;
      lv.u = raw[j];
#pragma unroll
      for (int i = 0; i < 8; ++i) key[j * 8 + i] = make_key(lv.s[i], off + i);
    } else {
      // the chunk's partial last vector (or nothing): guarded 2-byte loads
#pragma unroll
      for (int i = 0; i < 8; ++i)
        key[j * 8 + i] = off + i < n ? make_key(src[off + i], off + i) : 0u;
    }
  }

  __shared__ uint32_t red_u[2][kLpThreads / kWave];
  __shared__ float red_f[kLpThreads / kWave];
  const int wave = tid >> 6;
  const bool lead = (tid & 63) == 0;
  int parity = 0;
  // block-wide max; the two LDS rows alternate so one barrier per call
  // is enough (a row is rewritten only after the barrier that follows
  // its last read)
  auto block_max = [&](uint32_t v) {
    v = wave_max_u32(v);
    if (lead) red_u[parity][wave] = v;
    __syncthreads();
    v = max(max(red_u[parity][0], red_u[parity][1]),
            max(red_u[parity][2], red_u[parity][3]));
    parity ^= 1;
    return v;
  };
  auto thread_max = [&]() {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < kLpKeys; ++i) t = max(t, key[i]);
    return t;
  };

  // chunk max doubles as the first top-k winner
  uint32_t win = block_max(thread_max());
  const float m = win ? mono16_to_f32(win >> 16) : -INFINITY;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kLpKeys; ++i) {
    const float v = mono16_to_f32(key[i] >> 16);
    if (key[i] != 0u && v > -INFINITY) s += __expf(v - m);
  }
  s = wave_sum(s);
  if (lead) red_f[wave] = s;
  __syncthreads();
  if (tid == 0) {
    float* st = stats + (int64_t(r) * n_split + split) * 2;
    st[0] = m;
    st[1] = (red_f[0] + red_f[1]) + (red_f[2] + red_f[3]);
  }

  // k rounds of block-wide max; each winner is removed from the one
  // thread that holds it (keys are distinct)
  uint64_t* out = cand + (int64_t(r) * n_split + split) * k;
  for (int j = 0; j < k; ++j) {
    if (tid == 0) out[j] = win ? widen_key(win, e0) : 0ull;
    if (j + 1 == k) break;
#pragma unroll
    for (int i = 0; i < kLpKeys; ++i)
      if (key[i] == win) key[i] = 0u;
    win = block_max(thread_max());
  }
}

__global__ __launch_bounds__(kWave)
void logprobs_final_kernel(const uint16_t* __restrict__ logits,
                           const int32_t* __restrict__ rows,
                           const int32_t* __restrict__ tokens,
                           const float* __restrict__ stats,
                           const uint64_t* __restrict__ cand,
                           float* __restrict__ chosen_lp,
                           float* __restrict__ top_lp,
                           int32_t* __restrict__ top_ids, int vocab,
                           int n_split, int k) {
  const int r = blockIdx.x;
  const int lane = threadIdx.x;
  const float* st = stats + int64_t(r) * n_split * 2;
  float m = -INFINITY;
  for (int s = lane; s < n_split; s += kWave) m = fmaxf(m, st[2 * s]);
  m = wave_max(m);
  float sum = 0.f;
  for (int s = lane; s < n_split; s += kWave) {
    const float ms = st[2 * s];
    if (ms > -INFINITY) sum += st[2 * s + 1] * __expf(ms - m);
  }
  const float log_sum = __logf(wave_sum(sum));
  if (lane == 0) {
    const float x =
        bf16_to_f32(logits[int64_t(rows[r]) * vocab + tokens[r]]);
    chosen_lp[r] = (x - m) - log_sum;
  }
  if (k == 0) return;

  // n_split*k candidates -> k.  Up to 512 sit in registers; beyond that
  // (vocab > ~200k at k = 20) each round re-reads them from the (L2
  // resident) workspace.  Either way round j is max{key < winner j-1}.
  const int n = n_split * k;
  const uint64_t* c = cand + int64_t(r) * n;
  const bool in_regs = n <= kWave * kLpCandRegs;
  uint64_t reg[kLpCandRegs];
#pragma unroll
  for (int q = 0; q < kLpCandRegs; ++q) {
    const int i = q * kWave + lane;
    reg[q] = (in_regs && i < n) ? c[i] : 0ull;
  }
  uint64_t prev = ~0ull;
  for (int j = 0; j < k; ++j) {
    uint64_t best = 0ull;
    if (in_regs) {
#pragma unroll
      for (int q = 0; q < kLpCandRegs; ++q)
        if (reg[q] < prev) best = max(best, reg[q]);
    } else {
      for (int i = lane; i < n; i += kWave) {
        const uint64_t key = c[i];
        if (key < prev) best = max(best, key);
      }
    }
    best = wave_max_u64(best);
    prev = best;
    if (lane == 0) {
      top_lp[int64_t(r) * k + j] = (key64_value(best) - m) - log_sum;
      top_ids[int64_t(r) * k + j] = 0x7fffffff - int(best & 0xffffffffu);
    }
  }
}

}  // namespace

int logprobs_n_split(int rows, int vocab) {
  // fill the chip like the sampler does, but never let a chunk outgrow
  // the 8192 logits one workgroup holds in registers
  const int fill = sample_n_split(rows);
  const int need = (vocab + kLpChunkMax - 1) / kLpChunkMax;
  return fill > need ? fill : (need > 1 ? need : 1);
}

void launch_token_logprobs(const uint16_t* logits, const int32_t* rows,
                           const int32_t* tokens, float* chosen_lp,
                           float* top_lp, int32_t* top_ids, int n_rows,
                           int vocab, int k, float* stats, uint64_t* cand,
                           int n_split, hipStream_t stream) {
  if (n_rows == 0) return;
  // multiple of 8 so every chunk of a row shares the row's alignment
  const int chunk = ((vocab + n_split - 1) / n_split + 7) & ~7;
  hipLaunchKernelGGL(logprobs_part_kernel, dim3(n_rows, n_split),
                     dim3(kLpThreads), 0, stream, logits, rows, stats, cand,
                     vocab, n_split, chunk, k);
  hipLaunchKernelGGL(logprobs_final_kernel, dim3(n_rows), dim3(kWave), 0,
                     stream, logits, rows, tokens, stats, cand, chosen_lp,
                     top_lp, top_ids, vocab, n_split, k);
}

}  // namespace rlli
