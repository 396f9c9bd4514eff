// MFMA causal prefill attention (flash-style online softmax): one tile
// body, two entry kernels that differ only in where K/V come from.
//
// Replaces the VALU v1 (prefill_attn.hip) on the matrix cores: ~37 TF/s
// VALU -> MFMA tiles.  Geometry per workgroup = (32-row q-chunk of one
// sequence, kv-head), 4 waves:
//   - each wave owns ONE of the (up to 4) query heads of the GQA group
//     for the SAME 32 q rows, so all waves share the same causal range
//     and the same K/V tiles (Llama-8B GROUP=4 uses all 4; GROUP=8
//     splits across 2 workgroups);
//   - per KV tile (KVBLK=64): K and V are staged cooperatively ONCE per
//     workgroup in one barrier pair — K row-major but XOR-swizzled
//     (byte ^= (row & (D/8-1)) << 4) so the QK^T B-fragment read (16
//     lanes, 16 rows, same columns) is bank-conflict-free, V as padded
//     V^T so the PV B fragment is a contiguous ds_read_b128;
//     QK^T = 2x4 S-tiles of mfma_f32_16x16x32 accumulated over D
//     (B fragment = 16 contiguous bf16 of a K row — no transpose
//     needed); online softmax on the C-layout fragments (row r lives in
//     one 16-lane shfl group); P goes to bf16 through a per-wave padded
//     LDS buffer and comes back in A-fragment layout.
//   - O accumulates in registers ([2 q-tiles][D/16][4] f32), normalized
//     and stored at the end.
//
// The tile works in sequence-relative terms: a chunk is (first batch
// row row0, sequence position pos0 of that row, row count nrows), its
// keys are positions 0 .. pos0 + nrows - 1, tiled from position 0.  A
// KV source hands out the K and V row pieces of one key position:
//   - BatchKV (prefill_mfma_kernel, forward_prefill): position p is row
//     seq_start + p of the packed in-batch qkv tensor, read raw.  Chunk
//     tables (t0 / seq_start / seq_end) are built host-side from
//     cu_seqlens.
//   - PagedKV (prefill_paged_kernel, chunked prefill and mixed
//     prefill/decode batches): position p is found through the block
//     table in the paged cache, so a chunk of Q attends over its
//     sequence's ENTIRE cached prefix plus the chunk itself (whose K/V
//     rope_kv_append just wrote).  Cache block row [phys, kvh, tok, 0:D]
//     is contiguous, so a piece is still one vector load per lane.
//     Per-chunk metadata (row0 / pos0 / nrows / block-table row) comes
//     from the engine.
// Key positions past the chunk's causal bound stage zeros and are
// masked to -inf before the softmax, so partial tail tiles never touch
// another sequence's rows or an unwritten cache slot.

#include "common.h"

#include <type_traits>

namespace rlli {

namespace {

using bf16x8_vec = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr float kNegInf = -1e30f;
constexpr int QBLK = 32;
constexpr int KVBLK = 64;
constexpr int PPAD = KVBLK + 8;   // padded row stride (elements) for P / V^T

// A KV source's load(p, d8, valid, k8, put_v) fetches columns d8 .. d8+7
// of the K and V rows of key position p: K comes back as 8 bf16 in k8,
// the 8 V elements go one by one to put_v(j, bf16), which scatters them
// into V^T.  Without `valid` it touches no memory and hands out zeros.
// V goes through a callback so that each element's conversion is followed
// at once by its LDS store; the compiler keeps that order, and with the
// eight stores grouped behind the conversions the fp8 kernel ran 1 %
// slower on 2048- and 8192-token sequences.

// K/V of the packed in-batch qkv tensor: two raw 16-byte loads.
struct BatchKV {
  const uint16_t* k;     // k / v columns of this kv head in the row of
  const uint16_t* v;     // sequence position 0
  int stride;
  template <typename PutV>
  DEV_INLINE void load(int p, int d8, bool valid, uint4& k8,
                       PutV put_v) const {
    bf16x8 piece;
    piece.u = k8 = uint4{0, 0, 0, 0};
    if (valid) {
      piece.u = *reinterpret_cast<const uint4*>(v + int64_t(p) * stride + d8);
      k8 = *reinterpret_cast<const uint4*>(k + int64_t(p) * stride + d8);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) put_v(j, piece.s[j]);
  }
};

// K/V of the paged cache, through the cache codec: fp8 converts to bf16
// HERE, so the LDS images and every MFMA fragment are unchanged.
template <typename KC>
struct PagedKV {
  const typename KC::elem* k_cache;
  const typename KC::elem* v_cache;
  const int32_t* bt;     // this sequence's block-table row
  int n_kv_heads, kvh, block_size, head_dim;
  template <typename PutV>
  DEV_INLINE void load(int p, int d8, bool valid, uint4& k8,
                       PutV put_v) const {
    // only the loads are conditional (the codec runs on zeros otherwise),
    // which keeps both loads of a piece in flight together
    typename KC::vec8 vraw = {};
    typename KC::vec8 kraw = {};
    if (valid) {
      const int phys = bt[p / block_size];
      const int64_t a =
          (int64_t(phys) * n_kv_heads + kvh) * block_size * head_dim +
          int64_t(p % block_size) * head_dim;
      vraw = *reinterpret_cast<const typename KC::vec8*>(v_cache + a + d8);
      kraw = *reinterpret_cast<const typename KC::vec8*>(k_cache + a + d8);
    }
    float vf8[8], kf8[8];
    KC::to_f32(vraw, vf8);
    KC::to_f32(kraw, kf8);
    bf16x8 kp;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      put_v(j, f32_to_bf16(vf8[j]));
      kp.s[j] = f32_to_bf16(kf8[j]);
    }
    k8 = kp.u;
  }
};

// One workgroup's work: query heads head0 .. head0 + heads_per_wg - 1
// (one per wave) of chunk (row0, pos0, nrows) against keys from `src`.
template <int D, typename KV>
DEV_INLINE void prefill_tile(const uint16_t* __restrict__ qkv,
                             uint16_t* __restrict__ out, const KV& src,
                             int row0, int pos0, int nrows, int head0,
                             int heads_per_wg, int n_q_heads,
                             int qkv_stride, float scale) {
  constexpr int CT = D / 16;            // output column tiles
  constexpr int DC = D / 32;            // k-dim chunks per S mfma

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int jcol = lane & 15;
  const int koct = lane >> 4;
  const bool active = wave < heads_per_wg;
  const int head = head0 + wave;               // if active

  // LDS: V^T [D][PPAD] + K [KVBLK][D] shared, per-wave P [QBLK][PPAD]
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint16_t* vt = reinterpret_cast<uint16_t*>(smem_raw);          // D*PPAD
  uint16_t* ks = vt + D * PPAD;                                  // KVBLK*D, swizzled
  uint16_t* p_lds = ks + KVBLK * D + wave * QBLK * PPAD;         // per wave

  // ---- load Q fragments: [2 q-tiles][DC] x 4 VGPR ----
  bf16x8_vec qf[2][DC];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      const int r = qt * 16 + jcol;
      uint4 raw = {0, 0, 0, 0};
      if (active && r < nrows)
        raw = *reinterpret_cast<const uint4*>(
            qkv + int64_t(row0 + r) * qkv_stride + head * D + dc * 32 +
            koct * 8);
      qf[qt][dc] = *reinterpret_cast<bf16x8_vec*>(&raw);
    }
  }

  f32x4 o_acc[2][CT];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) o_acc[qt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  // softmax state: this lane's 4 rows per q-tile (row = koct*4 + reg)
  float m_st[2][4], l_st[2][4];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m_st[qt][r] = kNegInf;
      l_st[qt][r] = 0.f;
    }

  // causal bound: the chunk's last q row attends up to its own position
  const int kv_hi = pos0 + nrows;

  for (int kv0 = 0; kv0 < kv_hi; kv0 += KVBLK) {
    // ---- cooperative staging: K[kv0..kv0+KVBLK][D] -> ks (swizzled),
    //      V[kv0..kv0+KVBLK][D] -> vt[D][PPAD] ----
    __syncthreads();   // previous tile's reads done before overwrite
    {
      constexpr int PIECES = KVBLK * D / 8 / 256;
#pragma unroll
      for (int pc = 0; pc < PIECES; ++pc) {
        const int idx = pc * 256 + threadIdx.x;
        const int kv = idx / (D / 8);
        const int d8 = (idx % (D / 8)) * 8;
        const int p = kv0 + kv;
        uint4 kraw;
        src.load(p, d8, p < kv_hi, kraw, [&](int j, uint16_t x) {
          vt[(d8 + j) * PPAD + kv] = x;
        });
        // K stays row-major but XOR-swizzled so the B-fragment read
        // (16 lanes, 16 different rows, same column range) is
        // bank-conflict-free (guide T2 / G4); mask by row length so the
        // XOR never escapes the row (D=64 rows are only 128 B)
        *reinterpret_cast<uint4*>(
            reinterpret_cast<char*>(ks) +
            (kv * D * 2 + ((d8 * 2) ^ ((kv & (D / 8 - 1)) << 4)))) = kraw;
      }
    }
    __syncthreads();

    // ---- S = Q K^T over this tile (2 x KVBLK/16 16x16 tiles) ----
    constexpr int KT = KVBLK / 16;
    f32x4 s_acc[2][KT];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) s_acc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        // B fragments from the swizzled LDS K tile (staged once per
        // workgroup instead of 4x-redundant scattered L2 reads)
        bf16x8_vec kf[DC];
        const int krow = kt * 16 + jcol;
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
          uint4 raw = *reinterpret_cast<const uint4*>(
              reinterpret_cast<const char*>(ks) +
              (krow * D * 2 +
               (((dc * 32 + koct * 8) * 2) ^ ((krow & (D / 8 - 1)) << 4))));
          kf[dc] = *reinterpret_cast<bf16x8_vec*>(&raw);
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int dc = 0; dc < DC; ++dc)
            s_acc[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                qf[qt][dc], kf[dc], s_acc[qt][kt], 0, 0, 0);
      }

      // ---- causal + bounds mask, online softmax, P -> LDS ----
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        float corr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qpos = pos0 + qt * 16 + koct * 4 + r;   // seq position
          float sv[KT];
          float mx = kNegInf;
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) {
            float s = s_acc[qt][kt][r] * scale;
            const int c = kv0 + kt * 16 + jcol;
            if (c > qpos || c >= kv_hi) s = kNegInf;
            sv[kt] = s;
            mx = fmaxf(mx, s);
          }
          // row max across the 16-lane group
#pragma unroll
          for (int off = 8; off > 0; off >>= 1)
            mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
          const float m_new = fmaxf(m_st[qt][r], mx);
          corr[r] = __expf(m_st[qt][r] - m_new);
          m_st[qt][r] = m_new;
          float rs = 0.f;
          // store P row (bf16) to the per-wave LDS buffer
          const int prow = qt * 16 + koct * 4 + r;
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) {
            const float p = __expf(sv[kt] - m_new);
            rs += p;
            p_lds[prow * PPAD + kt * 16 + jcol] = f32_to_bf16(p);
          }
#pragma unroll
          for (int off = 8; off > 0; off >>= 1)
            rs += __shfl_xor(rs, off, kWave);
          l_st[qt][r] = l_st[qt][r] * corr[r] + rs;
        }
        // rescale O accumulators for this q-tile
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) o_acc[qt][ct][r] *= corr[r];
      }

      // ---- PV: A = P (from LDS, A-frag layout), B = V^T rows ----
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
        for (int kb = 0; kb < KVBLK / 32; ++kb) {
          uint4 praw = *reinterpret_cast<const uint4*>(
              p_lds + (qt * 16 + jcol) * PPAD + kb * 32 + koct * 8);
          bf16x8_vec pfrag = *reinterpret_cast<bf16x8_vec*>(&praw);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            uint4 vraw = *reinterpret_cast<const uint4*>(
                vt + (ct * 16 + jcol) * PPAD + kb * 32 + koct * 8);
            bf16x8_vec vfrag = *reinterpret_cast<bf16x8_vec*>(&vraw);
            o_acc[qt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pfrag, vfrag, o_acc[qt][ct], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- epilogue: normalize and store ----
  if (active) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = qt * 16 + koct * 4 + r;
        if (rr >= nrows) continue;
        const float inv_l = l_st[qt][r] > 0.f ? 1.f / l_st[qt][r] : 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          out[int64_t(row0 + rr) * n_q_heads * D + head * D + ct * 16 + jcol] =
              f32_to_bf16(o_acc[qt][ct][r] * inv_l);
      }
    }
  }
}

// blockIdx.x = (chunk, kv head, half of the GQA group when group > 4)
struct WgId {
  int chunk, kvh, head0, heads_per_wg;
  DEV_INLINE WgId(int n_kv_heads, int group, int n_hw) {
    chunk = blockIdx.x / (n_kv_heads * n_hw);
    kvh = (blockIdx.x / n_hw) % n_kv_heads;
    heads_per_wg = group / n_hw;               // <= 4
    head0 = kvh * group + (blockIdx.x % n_hw) * heads_per_wg;
  }
};

template <int D>
__global__ __launch_bounds__(256, 2)
void prefill_mfma_kernel(const uint16_t* __restrict__ qkv,
                         const int32_t* __restrict__ chunk_t0,
                         const int32_t* __restrict__ chunk_seq_start,
                         const int32_t* __restrict__ chunk_seq_end,
                         uint16_t* __restrict__ out,
                         int n_kv_heads, int group, int n_hw,
                         int qkv_stride, float scale) {
  const WgId wg(n_kv_heads, group, n_hw);
  const int t0 = chunk_t0[wg.chunk];
  const int seq_start = chunk_seq_start[wg.chunk];
  const int seq_end = chunk_seq_end[wg.chunk];
  const int n_q_heads = n_kv_heads * group;
  // k then v slices follow the q heads in a qkv row
  const uint16_t* k0 = qkv + int64_t(seq_start) * qkv_stride +
                       (n_q_heads + wg.kvh) * D;
  const BatchKV src{k0, k0 + n_kv_heads * D, qkv_stride};
  prefill_tile<D>(qkv, out, src, t0, t0 - seq_start,
                  min(QBLK, seq_end - t0), wg.head0, wg.heads_per_wg,
                  n_q_heads, qkv_stride, scale);
}

template <int D, typename KC>
__global__ __launch_bounds__(256, 2)
void prefill_paged_kernel(const uint16_t* __restrict__ qkv,
                          const typename KC::elem* __restrict__ k_cache,
                          const typename KC::elem* __restrict__ v_cache,
                          const int32_t* __restrict__ chunk_row0,
                          const int32_t* __restrict__ chunk_pos0,
                          const int32_t* __restrict__ chunk_nrows,
                          const int32_t* __restrict__ chunk_btrow,
                          const int32_t* __restrict__ block_tables,
                          uint16_t* __restrict__ out,
                          int n_kv_heads, int group, int n_hw,
                          int qkv_stride, int max_blocks, int block_size,
                          float scale) {
  const WgId wg(n_kv_heads, group, n_hw);
  const PagedKV<KC> src{
      k_cache, v_cache,
      block_tables + int64_t(chunk_btrow[wg.chunk]) * max_blocks,
      n_kv_heads, wg.kvh, block_size, D};
  prefill_tile<D>(qkv, out, src, chunk_row0[wg.chunk], chunk_pos0[wg.chunk],
                  chunk_nrows[wg.chunk], wg.head0, wg.heads_per_wg,
                  n_kv_heads * group, qkv_stride, scale);
}

// Grid and dynamic-LDS size, the same for both entries.
struct TileLaunch {
  int n_hw, blocks;
  size_t smem;
  TileLaunch(int n_chunks, int n_kv_heads, int group, int head_dim)
      : n_hw(group > 4 ? group / 4 : 1),
        blocks(n_chunks * n_kv_heads * n_hw),
        smem(size_t(head_dim) * PPAD * 2 + size_t(KVBLK) * head_dim * 2 +
             size_t(4) * QBLK * PPAD * 2) {}
};

}  // namespace

void launch_prefill_mfma(const uint16_t* qkv, const int32_t* chunk_t0,
                         const int32_t* chunk_seq_start,
                         const int32_t* chunk_seq_end, uint16_t* out,
                         int n_chunks, int n_kv_heads, int group,
                         int head_dim, int qkv_stride, float scale,
                         hipStream_t stream) {
  const TileLaunch l(n_chunks, n_kv_heads, group, head_dim);
  auto go = [&](auto d_tag) {
    hipLaunchKernelGGL(prefill_mfma_kernel<decltype(d_tag)::value>,
                       dim3(l.blocks), dim3(256), l.smem, stream, qkv,
                       chunk_t0, chunk_seq_start, chunk_seq_end, out,
                       n_kv_heads, group, l.n_hw, qkv_stride, scale);
  };
  if (head_dim == 128) go(std::integral_constant<int, 128>{});
  else if (head_dim == 64) go(std::integral_constant<int, 64>{});
}

void launch_prefill_paged(const uint16_t* qkv, const void* k_cache,
                          const void* v_cache, const int32_t* chunk_row0,
                          const int32_t* chunk_pos0,
                          const int32_t* chunk_nrows,
                          const int32_t* chunk_btrow,
                          const int32_t* block_tables, uint16_t* out,
                          int n_chunks, int n_kv_heads, int group,
                          int head_dim, int qkv_stride, int max_blocks,
                          int block_size, float scale, bool cache_fp8,
                          hipStream_t stream) {
  const TileLaunch l(n_chunks, n_kv_heads, group, head_dim);
  auto go = [&](auto d_tag, auto kc_tag) {
    using KC = decltype(kc_tag);
    hipLaunchKernelGGL((prefill_paged_kernel<decltype(d_tag)::value, KC>),
                       dim3(l.blocks), dim3(256), l.smem, stream, qkv,
                       static_cast<const typename KC::elem*>(k_cache),
                       static_cast<const typename KC::elem*>(v_cache),
                       chunk_row0, chunk_pos0, chunk_nrows, chunk_btrow,
                       block_tables, out, n_kv_heads, group, l.n_hw,
                       qkv_stride, max_blocks, block_size, scale);
  };
  using D128 = std::integral_constant<int, 128>;
  using D64 = std::integral_constant<int, 64>;
  if (head_dim == 128) {
    if (cache_fp8) go(D128{}, CacheFP8{}); else go(D128{}, CacheBF16{});
  } else if (head_dim == 64) {
    if (cache_fp8) go(D64{}, CacheFP8{}); else go(D64{}, CacheBF16{});
  }
}

}  // namespace rlli
