// Device helpers shared by the sampler kernels (sampling.hip) and the
// nucleus/penalty sampler (sampling_nucleus.hip): the counter-based
// uniform, the per-element score, the biased row walk and the radix-
// select bin search.  One definition, so every sampler picks the same
// token for the same (value, seed, index).
#pragma once

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

// bias of token idx in ids[0, n) (ascending); 0 when it has none
DEV_INLINE float find_bias(const int32_t* __restrict__ ids,
                           const float* __restrict__ vals, int n, int idx) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < idx) lo = mid + 1; else hi = mid;
  }
  return ids[lo] == idx ? vals[lo] : 0.f;
}

// f(z, idx) for every token of the row this thread owns, z being the
// logit, or adj(logit, idx) for a token whose bit is set in the one-bit-
// per-token LDS bitmap (consulted only when `marked`; one byte per bf16x8
// vector); two vectors in flight per lane before any arithmetic
template <typename A, typename F>
DEV_INLINE void scan_marked_row(const uint16_t* __restrict__ lrow, int vocab,
                                uint32_t mis, const uint32_t* bitmap,
                                bool marked, A&& adj, F&& f) {
  const int nvec = vocab / 8;
  auto one_vec = [&](uint4 raw, int v) {
    bf16x8 lv;
    lv.u = raw;
    const uint32_t hit =
        marked ? (bitmap[v >> 2] >> ((v & 3) * 8)) & 0xffu : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float z = bf16_to_f32(lv.s[i]);
      if (hit >> i & 1u) z = adj(z, v * 8 + i);
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
    if (marked && (bitmap[idx >> 5] >> (idx & 31) & 1u)) z = adj(z, idx);
    f(z, idx);
  }
}

// the walk with z = logit + bias: the bitmap marks the ids of the row's
// ascending bias list, and only a hit searches it
template <typename F>
DEV_INLINE void scan_biased_row(const uint16_t* __restrict__ lrow, int vocab,
                                uint32_t mis, const uint32_t* bitmap,
                                const int32_t* __restrict__ ids,
                                const float* __restrict__ vals, int n_bias,
                                F&& f) {
  scan_marked_row(
      lrow, vocab, mis, bitmap, n_bias > 0,
      [&](float z, int idx) { return z + find_bias(ids, vals, n_bias, idx); },
      f);
}

DEV_INLINE uint32_t shfl_up_acc(uint32_t v, int off) {
  return uint32_t(__shfl_up(int(v), off, kWave));
}

using u64acc = unsigned long long;              // what 64-bit LDS adds take

DEV_INLINE u64acc shfl_up_acc(u64acc v, int off) {
  const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), off, kWave));
  const uint32_t hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), off, kWave));
  return u64acc(hi) << 32 | lo;
}

// Wave 0: the highest bin at which the total from the top reaches *need.
// Lane l sums the l-th group of bins from the top; the lane whose group
// crosses walks it.  Leaves the bin in *sel and what is still needed
// inside it in *need.  T is the accumulator: uint32_t counts for the
// k-th largest value, u64acc fixed-point weights for the nucleus.
template <typename T>
DEV_INLINE void select_bin(const T* hist, int n_bins, uint32_t* sel,
                           T* need) {
  const int lane = threadIdx.x;
  const int per = n_bins / kWave;
  const int top = n_bins - 1 - lane * per;       // this lane's highest bin
  T own = 0;
  // rotated start: lanes' bins are `per` words apart, which would put
  // them all in one bank
  for (int i = 0; i < per; ++i) own += hist[top - ((i + lane) & (per - 1))];
  T incl = own;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T o = shfl_up_acc(incl, off);
    if (lane >= off) incl += o;
  }
  const T k = *need;
  const uint64_t crossed = __ballot(incl >= k);
  if (crossed != 0 && lane == __ffsll((long long)crossed) - 1) {
    T above = incl - own;
    int b = top;
    for (int i = 0; i < per - 1 && above + hist[b] < k; ++i, --b)
      above += hist[b];
    *sel = uint32_t(b);
    *need = k - above;
  }
}

}  // namespace

}  // namespace rlli
