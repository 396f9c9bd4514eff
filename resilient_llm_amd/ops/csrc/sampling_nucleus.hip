// Nucleus (top_p) filtering and presence/frequency penalties on the
// device, next to sample_constrained_kernel and with its walk, score and
// radix select (sampling_common.h).
//
// One 1024-thread workgroup per SELECTED row.  With c(t) the number of
// times token t occurs in the row's device-resident history,
//   z(t) = float(logit) - (presence + frequency * float(c))  [c > 0]
//                       + bias(t)                             (f32, this order)
//   setup       LDS hash table token -> count from the history (open
//               addressing, 18-bit id | 14-bit count per word), and one
//               bitmap bit per token that has a count or a bias: a row
//               walk pays a lookup only for those
//   walk 1      z_max (+ the top-digit count histogram when top_k is on)
//   walk 2, 3   the other two digits of the k-th largest z   (top_k only)
//   walk 4-6    the nucleus cut: the three 11/11/10-bit digits of the
//               smallest kept z, by a radix select over per-bin MASS.  A
//               token weighs uint64(exp((z - z_max)/T) * 2^32), summed by
//               64-bit LDS integer adds, so the mass is independent of
//               the order of the adds and repeated calls are bit-identical.
//               Only survivors of top_k / min_p weigh; W is their total and
//               the target is ceil(top_p * W) in the same fixed point
//   last walk   Gumbel arg-max of sample_score over z >= the cut
// The top_k walks and the mass walks run in sequence: W is the mass of the
// top_k survivors, which is not known before the k-th value is.  Walks
// per sampled row: 1 plain, 2 min_p, 4 top_k, 5 top_p (+ min_p), 7 top_k +
// top_p; greedy rows always walk once.  Thread 0 appends the chosen token
// to the row's history slot with plain stores.  The logits are only read;
// nothing goes through global atomics.
//
// LDS: bitmap 32 KB + hash table 32 KB + count histogram 8 KB + mass
// histogram 16 KB + reductions < 1 KB = 88.3 KB of the 160 KB.

#include "sampling_common.h"

namespace rlli {

namespace {

constexpr int kNucMaxHistory = 4096;
constexpr int kNucTable = 2 * kNucMaxHistory;    // load factor <= 1/2
constexpr uint32_t kNucEmpty = 0xffffffffu;      // id 2^18-1 with count 2^14-1:
                                                 // no count gets that far

DEV_INLINE uint32_t nuc_home(uint32_t tok) {
  return (tok * 0x9e3779b1u) >> 19;              // 13 bits
}

DEV_INLINE void nuc_insert(uint32_t* table, uint32_t tok) {
  uint32_t h = nuc_home(tok);
  // at most kNucMaxHistory distinct ids in 2x as many entries: ends
  for (;;) {
    const uint32_t old = atomicCAS(&table[h], kNucEmpty, tok << 14);
    if (old == kNucEmpty || old >> 14 == tok) {
      atomicAdd(&table[h], 1u);
      return;
    }
    h = (h + 1) & (kNucTable - 1);
  }
}

DEV_INLINE uint32_t nuc_count(const uint32_t* table, uint32_t tok) {
  uint32_t h = nuc_home(tok);
  for (;;) {
    const uint32_t e = table[h];
    if (e == kNucEmpty) return 0u;
    if (e >> 14 == tok) return e & 0x3fffu;
    h = (h + 1) & (kNucTable - 1);
  }
}

DEV_INLINE u64acc wave_sum_u64(u64acc v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(v)), off, kWave));
    const uint32_t hi =
        uint32_t(__shfl_xor(int(uint32_t(v >> 32)), off, kWave));
    v += u64acc(hi) << 32 | lo;
  }
  return v;
}

__global__ __launch_bounds__(kCsThreads)
void sample_nucleus_kernel(const uint16_t* __restrict__ logits,
                           const int32_t* __restrict__ rows,
                           const float* __restrict__ temperatures,
                           const uint64_t* __restrict__ seeds, uint64_t step,
                           const int32_t* __restrict__ top_k,
                           const float* __restrict__ min_p,
                           const float* __restrict__ top_p,
                           const float* __restrict__ presence,
                           const float* __restrict__ frequency,
                           const int32_t* __restrict__ bias_offsets,
                           const int32_t* __restrict__ bias_ids,
                           const float* __restrict__ bias_vals,
                           int n_bias_total,
                           const int32_t* __restrict__ hist_slot,
                           int32_t* history, int32_t* hist_len, int n_slots,
                           int cap, int append,
                           int32_t* __restrict__ out_tokens, int vocab) {
  __shared__ uint32_t bitmap[kCsMaxVocab / 32];
  __shared__ uint32_t table[kNucTable];
  __shared__ uint32_t hist[kCsBins];
  __shared__ u64acc mass[kCsBins];
  __shared__ u64acc red_mass[kCsWaves];
  __shared__ float red_val[kCsWaves];
  __shared__ int red_idx[kCsWaves];
  __shared__ uint32_t sel_bin, sel_need;
  __shared__ u64acc sel_mass;

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

  // the row's history slot, clamped likewise
  int slot = hist_slot[r];
  if (slot < 0 || slot >= n_slots) slot = -1;
  const int len = slot >= 0 ? hist_len[slot] : 0;
  const int n_hist = min(max(len, 0), cap);
  int32_t* hrow = history + int64_t(max(slot, 0)) * cap;
  const float pres = presence[r];
  const float freq = frequency[r];
  const bool pen = n_hist > 0 && (pres != 0.f || freq != 0.f);

  const bool marked = n_bias > 0 || pen;
  if (marked) {
    for (int i = tid; i < (vocab + 31) / 32; i += kCsThreads) bitmap[i] = 0u;
    if (pen)
      for (int i = tid; i < kNucTable; i += kCsThreads) table[i] = kNucEmpty;
    __syncthreads();
    for (int i = tid; i < n_bias; i += kCsThreads) {
      const int id = ids[i];
      if (id >= 0 && id < vocab) atomicOr(&bitmap[id >> 5], 1u << (id & 31));
    }
    if (pen) {
      for (int i = tid; i < n_hist; i += kCsThreads) {
        const int id = hrow[i];
        if (id >= 0 && id < vocab) {
          atomicOr(&bitmap[id >> 5], 1u << (id & 31));
          nuc_insert(table, uint32_t(id));
        }
      }
    }
    __syncthreads();
  }
  auto scan = [&](auto&& f) {
    scan_marked_row(
        lrow, vocab, mis, bitmap, marked,
        [&](float z, int idx) {
          if (pen) {
            const uint32_t c = nuc_count(table, uint32_t(idx));
            // one penalty term, subtracted before the bias goes on; the
            // explicit roundings keep the compiler from fusing across it
            if (c != 0u)
              z = __fsub_rn(z, __fadd_rn(pres, __fmul_rn(freq, float(c))));
          }
          if (n_bias > 0) z += find_bias(ids, vals, n_bias, idx);
          return z;
        },
        f);
  };

  const int k = top_k[r];
  const float mp = min_p[r];
  const float tp = top_p[r];
  const bool use_k = !greedy && k >= 1 && k < vocab;
  const bool use_p = !greedy && mp > 0.f;
  const bool use_n = !greedy && tp > 0.f && tp < 1.f;
  float thr = -INFINITY;
  if (tid == 0) sel_bin = 0u;
  if (use_k || use_p || use_n) {
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
    if (use_n) {
      // digits of the smallest kept key: from the top, the first value
      // at which the survivors' mass, itself included, reaches top_p * W
      auto weight = [&](float z) {
        return u64acc(__expf((z - zmax) * inv_t) * 4294967296.f);
      };
      for (int i = tid; i < kCsBins; i += kCsThreads) mass[i] = 0ull;
      __syncthreads();
      u64acc total = 0ull;
      scan([&](float z, int) {
        if (z >= thr) {
          const u64acc w = weight(z);
          total += w;
          atomicAdd(&mass[mono32(z) >> 21], w);
        }
      });
      total = wave_sum_u64(total);
      if ((tid & 63) == 0) red_mass[tid >> 6] = total;
      __syncthreads();
      if (tid == 0) {
        u64acc W = 0ull;
        for (int w = 0; w < kCsWaves; ++w) W += red_mass[w];
        const u64acc want = u64acc(ceil(double(tp) * double(W)));
        sel_mass = min(max(want, u64acc(1)), W);
      }
      __syncthreads();
      if (tid < kWave) select_bin(mass, kCsBins, &sel_bin, &sel_mass);
      __syncthreads();
      uint32_t prefix = sel_bin;                    // key >> 21
      for (int i = tid; i < kCsBins; i += kCsThreads) mass[i] = 0ull;
      __syncthreads();
      scan([&](float z, int) {
        const uint32_t key = mono32(z);
        if (z >= thr && key >> 21 == prefix)
          atomicAdd(&mass[key >> 10 & 2047u], weight(z));
      });
      __syncthreads();
      if (tid < kWave) select_bin(mass, kCsBins, &sel_bin, &sel_mass);
      __syncthreads();
      prefix = prefix << 11 | sel_bin;              // key >> 10
      for (int i = tid; i < 1024; i += kCsThreads) mass[i] = 0ull;
      __syncthreads();
      scan([&](float z, int) {
        const uint32_t key = mono32(z);
        if (z >= thr && key >> 10 == prefix)
          atomicAdd(&mass[key & 1023u], weight(z));
      });
      __syncthreads();
      if (tid < kWave) select_bin(mass, 1024, &sel_bin, &sel_mass);
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
    // every thread has long finished reading the history (the hash table
    // was built before the first walk)
    if (append != 0 && slot >= 0 && len >= 0 && len < cap) {
      hrow[len] = fb.idx;
      hist_len[slot] = len + 1;
    }
  }
}

}  // namespace

int sample_nucleus_max_history() { return kNucMaxHistory; }

void launch_sample_nucleus(const uint16_t* logits, const int32_t* rows,
                           const float* temperatures, const uint64_t* seeds,
                           uint64_t step, const int32_t* top_k,
                           const float* min_p, const float* top_p,
                           const float* presence, const float* frequency,
                           const int32_t* bias_offsets,
                           const int32_t* bias_ids, const float* bias_vals,
                           int n_bias_total, const int32_t* hist_slot,
                           int32_t* history, int32_t* hist_len, int n_slots,
                           int cap, bool append, int32_t* out_tokens,
                           int n_rows, int vocab, hipStream_t stream) {
  if (n_rows == 0) return;
  hipLaunchKernelGGL(sample_nucleus_kernel, dim3(n_rows), dim3(kCsThreads), 0,
                     stream, logits, rows, temperatures, seeds, step, top_k,
                     min_p, top_p, presence, frequency, bias_offsets,
                     bias_ids, bias_vals, n_bias_total, hist_slot, history,
                     hist_len, n_slots, cap, append ? 1 : 0, out_tokens,
                     vocab);
}

}  // namespace rlli
