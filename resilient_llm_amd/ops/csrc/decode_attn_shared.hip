// Shared-prefix decode attention: sequences of one decode batch that
// share a leading run of physical KV blocks (n > 1 choices of one prompt,
// prefix-cache hits on one system prompt) read that run ONCE per group.
//
// decode_attn_kernel streams every sequence's whole chain, so a prompt
// shared by 16 rows crosses HBM 16 times per layer per step.  Here the
// work is cut in two:
//
// 1. shared_prefix_attn_kernel (MFMA).  A row tile is up to 64 query rows
//    = 64/GROUP member sequences x the GROUP heads of one kv-head, enough
//    to fill 16x16x32 bf16 MFMAs where one sequence's GROUP rows cannot.
//    Grid = (row tile, kv-head, chunk of the prefix); 4 waves, each owns
//    16 rows whose Q A-fragments stay in registers.  The workgroup walks
//    its chunk in KV tiles of 64 tokens (4 cache blocks of the group's
//    block list):
//      - global -> registers for tile t+1 is issued before the math of
//        tile t, so HBM latency hides behind the MFMAs;
//      - K goes to LDS row-major, 16-byte pieces XOR-swizzled by row so
//        the QK^T B-fragment read (16 lanes, 16 rows, one column range)
//        is conflict-free;
//      - V goes to LDS transposed, V^T[d][token].  A thread takes the
//        SAME 8 dims of two adjacent tokens and stores 8 packed
//        (token, token+1) dwords; the 16-byte token chunks of row d sit
//        at chunk ^ (d >> 4), which spreads the 16 rows x 4 token pairs
//        one store instruction touches over all 64 banks, and leaves the
//        PV B-fragment a single aligned 16-byte read;
//      - S = Q K^T, online softmax on the C-layout fragments (no causal
//        mask: every prefix key is visible to every row), P -> per-wave
//        LDS tile as bf16 -> A fragments, O += P V.
//    The result is NOT normalised: f32 partials (acc, m, l) per (tile,
//    kv-head, chunk, row) go to a workspace.  An empty chunk (the group's
//    prefix is shorter than the longest one) writes l = 0.
//
// 2. shared_suffix_merge_kernel (vector).  One workgroup per (sequence,
//    kv-head) for EVERY row of the batch, decode_attn_kernel's lane-group
//    scheme over the row's private blocks n_shared/16 .. (the appended
//    token included), then a log-sum-exp fold of the row's prefix
//    partials over all chunks, normalise, bf16 out.  A row in no group
//    has n_shared = 0: for it this is a complete decode attention, with
//    no split-K.
//
// Only bytes below seq_len reach the result: cache slots past it weigh
// zero whatever they hold, block-table entries past the chain and the
// blocks they would name are never read.
// bf16 cache, block size 16, head_dim 128, GROUP 4 or 8.

#include "common.h"

#include <type_traits>

namespace rlli {

namespace {

using bf16x8_vec = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr float kNegInf = -1e30f;
constexpr int D = 128;
constexpr int BS = 16;                // cache block size
constexpr int KVT = 64;               // tokens per KV tile (4 cache blocks)
constexpr int TROWS = 64;             // query rows per row tile
constexpr int PPAD = KVT + 8;         // row stride (elements) of V^T and P
constexpr int CT = D / 16;            // output column tiles
constexpr int DC = D / 32;            // k-dim steps of one S tile
constexpr int KT = KVT / 16;          // S tiles per KV tile
constexpr int kMaxChunks = 64;        // the wrapper rejects more

// byte offset of the 16-byte piece (row kv, columns d8 .. d8+7) in the
// swizzled K tile
DEV_INLINE int k_off(int kv, int d8) {
  return kv * D * 2 + ((d8 * 2) ^ ((kv & 15) << 4));
}
// element offset of (row d, token chunk c = token / 8) in swizzled V^T
DEV_INLINE int vt_off(int d, int c) {
  return d * PPAD + ((c ^ ((d >> 4) & 7)) << 3);
}

template <int GROUP>
__global__ __launch_bounds__(256, 2)
void shared_prefix_attn_kernel(const uint16_t* __restrict__ qkv,
                               const uint16_t* __restrict__ k_cache,
                               const uint16_t* __restrict__ v_cache,
                               const int32_t* __restrict__ block_table,
                               const int32_t* __restrict__ tile_rows,
                               const int32_t* __restrict__ tile_blocks,
                               const int32_t* __restrict__ tile_bt_row,
                               float* __restrict__ ws_acc,
                               float* __restrict__ ws_ml,
                               int n_kv_heads, int max_blocks, int q_stride,
                               float scale) {
  constexpr int MPT = TROWS / GROUP;          // members per tile
  const int tile = blockIdx.x;
  const int kvh = blockIdx.y;
  const int chunk = blockIdx.z;
  const int n_chunks = gridDim.z;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int jcol = lane & 15;
  const int koct = lane >> 4;

  __shared__ __attribute__((aligned(16))) uint16_t vt[D * PPAD];
  __shared__ __attribute__((aligned(16))) uint16_t ks[KVT * D];
  __shared__ __attribute__((aligned(16))) uint16_t p_all[4 * 16 * PPAD];
  uint16_t* p_lds = p_all + wave * 16 * PPAD;

  const int nb = tile_blocks[tile];           // shared blocks, all full
  const int n_kvt = (nb * BS + KVT - 1) / KVT;
  const int per_chunk = (n_kvt + n_chunks - 1) / n_chunks;
  const int t_begin = chunk * per_chunk;
  const int t_end = min(t_begin + per_chunk, n_kvt);
  const int32_t* bl = block_table + int64_t(tile_bt_row[tile]) * max_blocks;

  // this lane's 4 C-layout rows belong to one member (GROUP >= 4)
  const int out_row0 = wave * 16 + koct * 4;
  const bool out_valid = tile_rows[tile * MPT + out_row0 / GROUP] >= 0;
  const int64_t part =
      ((int64_t(tile) * n_kv_heads + kvh) * n_chunks + chunk) * TROWS;

  if (t_begin >= t_end) {     // nothing of the prefix here: a zero partial
    if (out_valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* dst = ws_acc + (part + out_row0 + r) * D;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) dst[ct * 16 + jcol] = 0.f;
        if (jcol == 0) {
          ws_ml[(part + out_row0 + r) * 2 + 0] = kNegInf;
          ws_ml[(part + out_row0 + r) * 2 + 1] = 0.f;
        }
      }
    }
    return;
  }

  // ---- Q A-fragments of this wave's 16 rows (zeros past the members) ----
  bf16x8_vec qf[DC];
  {
    const int row = wave * 16 + jcol;
    const int brow = tile_rows[tile * MPT + row / GROUP];
    const int head = kvh * GROUP + row % GROUP;
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      uint4 raw = {0, 0, 0, 0};
      if (brow >= 0)
        raw = *reinterpret_cast<const uint4*>(
            qkv + int64_t(brow) * q_stride + head * D + dc * 32 + koct * 8);
      qf[dc] = *reinterpret_cast<bf16x8_vec*>(&raw);
    }
  }

  f32x4 o_acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) o_acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_st[4], l_st[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_st[r] = kNegInf;
    l_st[r] = 0.f;
  }

  // ---- staging registers: 4 K pieces (one per cache block of the tile)
  //      and 2 x 2 V pieces (the same 8 dims of two adjacent tokens) ----
  const int st_tok = tid >> 4;                // 0..15
  const int st_d8 = (tid & 15) * 8;
  uint4 kreg[4], vreg[4];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) {
      const int b = t * 4 + pc;
      kreg[pc] = uint4{0, 0, 0, 0};
      if (b < nb) {
        const int64_t a = (int64_t(bl[b]) * n_kv_heads + kvh) * (BS * D) +
                          st_tok * D + st_d8;
        kreg[pc] = *reinterpret_cast<const uint4*>(k_cache + a);
      }
    }
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int tok0 = (pc * 16 + st_tok) * 2;        // even token of the pair
      const int b = t * 4 + tok0 / BS;
      vreg[2 * pc] = vreg[2 * pc + 1] = uint4{0, 0, 0, 0};
      if (b < nb) {
        const int64_t a = (int64_t(bl[b]) * n_kv_heads + kvh) * (BS * D) +
                          (tok0 % BS) * D + st_d8;
        vreg[2 * pc] = *reinterpret_cast<const uint4*>(v_cache + a);
        vreg[2 * pc + 1] = *reinterpret_cast<const uint4*>(v_cache + a + D);
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int pc = 0; pc < 4; ++pc)
      *reinterpret_cast<uint4*>(reinterpret_cast<char*>(ks) +
                                k_off(pc * 16 + st_tok, st_d8)) = kreg[pc];
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int kv2 = pc * 16 + st_tok;               // token pair
      const bf16x8* v0 = reinterpret_cast<const bf16x8*>(&vreg[2 * pc]);
      const bf16x8* v1 = reinterpret_cast<const bf16x8*>(&vreg[2 * pc + 1]);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<uint32_t*>(
            vt + vt_off(st_d8 + j, kv2 >> 2) + (kv2 & 3) * 2) =
            uint32_t(v0->s[j]) | (uint32_t(v1->s[j]) << 16);
    }
  };

  const int n_tok = nb * BS;
  load_tile(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();          // the previous tile's fragment reads are done
    store_tile();
    __syncthreads();
    if (t + 1 < t_end) load_tile(t + 1);

    // ---- S = Q K^T: 4 tiles of 16 rows x 16 keys ----
    f32x4 s_acc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      s_acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int krow = kt * 16 + jcol;
#pragma unroll
      for (int dc = 0; dc < DC; ++dc) {
        uint4 raw = *reinterpret_cast<const uint4*>(
            reinterpret_cast<const char*>(ks) +
            k_off(krow, dc * 32 + koct * 8));
        s_acc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            qf[dc], *reinterpret_cast<bf16x8_vec*>(&raw), s_acc[kt], 0, 0, 0);
      }
    }

    // ---- online softmax; row koct*4 + r lives in one 16-lane group ----
    float corr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sv[KT];
      float mx = kNegInf;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const int c = t * KVT + kt * 16 + jcol;
        sv[kt] = c < n_tok ? s_acc[kt][r] * scale : kNegInf;
        mx = fmaxf(mx, sv[kt]);
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1)
        mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
      const float m_new = fmaxf(m_st[r], mx);
      corr[r] = __expf(m_st[r] - m_new);
      m_st[r] = m_new;
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const float p = __expf(sv[kt] - m_new);
        rs += p;
        p_lds[(koct * 4 + r) * PPAD + kt * 16 + jcol] = f32_to_bf16(p);
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) rs += __shfl_xor(rs, off, kWave);
      l_st[r] = l_st[r] * corr[r] + rs;
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[ct][r] *= corr[r];

    // ---- O += P V: A = P rows from LDS, B = V^T rows ----
#pragma unroll
    for (int kb = 0; kb < KVT / 32; ++kb) {
      uint4 praw = *reinterpret_cast<const uint4*>(
          p_lds + jcol * PPAD + kb * 32 + koct * 8);
      const bf16x8_vec pfrag = *reinterpret_cast<bf16x8_vec*>(&praw);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        uint4 vraw = *reinterpret_cast<const uint4*>(
            vt + vt_off(ct * 16 + jcol, kb * 4 + koct));
        o_acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pfrag, *reinterpret_cast<bf16x8_vec*>(&vraw), o_acc[ct], 0, 0, 0);
      }
    }
  }

  // ---- unnormalised partials of the member rows ----
  if (out_valid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* dst = ws_acc + (part + out_row0 + r) * D;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) dst[ct * 16 + jcol] = o_acc[ct][r];
      if (jcol == 0) {
        ws_ml[(part + out_row0 + r) * 2 + 0] = m_st[r];
        ws_ml[(part + out_row0 + r) * 2 + 1] = l_st[r];
      }
    }
  }
}

// Suffix phase: decode_attn_kernel's scheme at GW = 16, block size 16 —
// a wave is 4 lane-groups of 16 lanes x 8 dims, a lane-group takes 4
// tokens of a cache block, a wave every 4th block, the next block's
// loads are in flight while this one computes.
template <int GROUP>
__global__ __launch_bounds__(256)
void shared_suffix_merge_kernel(const uint16_t* __restrict__ qkv,
                                const uint16_t* __restrict__ k_cache,
                                const uint16_t* __restrict__ v_cache,
                                const int32_t* __restrict__ block_table,
                                const int32_t* __restrict__ seq_lens,
                                const int32_t* __restrict__ n_shared,
                                const int32_t* __restrict__ row_tile,
                                const int32_t* __restrict__ row_slot,
                                const float* __restrict__ ws_acc,
                                const float* __restrict__ ws_ml,
                                uint16_t* __restrict__ out,
                                int n_kv_heads, int max_blocks, int n_chunks,
                                float scale, int q_stride) {
  constexpr int GW = 16;
  constexpr int GPW = 64 / GW;                // lane-groups per wave
  constexpr int TPG = BS / GPW;               // tokens per lane-group
  const int seq = blockIdx.x / n_kv_heads;
  const int kvh = blockIdx.x % n_kv_heads;
  const int len = seq_lens[seq];
  const int shared_tok = n_shared[seq];       // a multiple of BS
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int group = lane / GW;
  const int gl = lane % GW;
  const int d0 = gl * 8;

  __shared__ float accs[4 * GROUP * D];       // [wave][GROUP][D]
  __shared__ float ml[4 * GROUP * 2];
  __shared__ float pml[kMaxChunks * GROUP * 2];   // prefix (m, l) per chunk

  float qv[GROUP][8];
#pragma unroll
  for (int h = 0; h < GROUP; ++h) {
    bf16x8 qh;
    qh.u = *reinterpret_cast<const uint4*>(
        qkv + int64_t(seq) * q_stride + (kvh * GROUP + h) * D + d0);
#pragma unroll
    for (int i = 0; i < 8; ++i) qv[h][i] = bf16_to_f32(qh.s[i]);
  }

  float m[GROUP], l[GROUP], acc[GROUP][8];
#pragma unroll
  for (int h = 0; h < GROUP; ++h) {
    m[h] = kNegInf;
    l[h] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[h][i] = 0.f;
  }

  const int n_blocks = (len + BS - 1) / BS;
  const int32_t* bt = block_table + int64_t(seq) * max_blocks;

  // a walked block is loaded whole (its tail past len is the row's own
  // allocated memory); consume_block drops what lies past len
  auto issue_block = [&](int phys, uint4 (&kraw)[TPG], uint4 (&vraw)[TPG]) {
    const int64_t kv_base = (int64_t(phys) * n_kv_heads + kvh) * (BS * D);
#pragma unroll
    for (int i = 0; i < TPG; ++i) {
      const int tok = group + GPW * i;
      kraw[i] = *reinterpret_cast<const uint4*>(
          k_cache + kv_base + tok * D + d0);
      vraw[i] = *reinterpret_cast<const uint4*>(
          v_cache + kv_base + tok * D + d0);
    }
  };
  // all TPG scores of a head before ONE running-max update; a walked
  // block holds at least one valid token, so m_new is finite
  auto consume_block = [&](int b, const uint4 (&kraw)[TPG],
                           const uint4 (&vraw)[TPG]) {
    float vfs[TPG][8];
    float svals[GROUP][TPG];
#pragma unroll
    for (int i = 0; i < TPG; ++i) {
      const bool valid = b * BS + group + GPW * i < len;
      float kf[8];
      CacheBF16::to_f32(kraw[i], kf);
      CacheBF16::to_f32(vraw[i], vfs[i]);
      // p = 0 does not silence a NaN/Inf left in an unwritten slot
#pragma unroll
      for (int j = 0; j < 8; ++j) vfs[i][j] = valid ? vfs[i][j] : 0.f;
#pragma unroll
      for (int h = 0; h < GROUP; ++h) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += qv[h][j] * kf[j];
        s = group_sum_dpp<GW>(s) * scale;
        svals[h][i] = valid ? s : kNegInf;
      }
    }
#pragma unroll
    for (int h = 0; h < GROUP; ++h) {
      float m_new = m[h];
#pragma unroll
      for (int i = 0; i < TPG; ++i) m_new = fmaxf(m_new, svals[h][i]);
      const float corr = __expf(m[h] - m_new);
      float p[TPG], psum = 0.f;
#pragma unroll
      for (int i = 0; i < TPG; ++i) {
        p[i] = __expf(svals[h][i] - m_new);
        psum += p[i];
      }
      m[h] = m_new;
      l[h] = l[h] * corr + psum;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = acc[h][j] * corr;
#pragma unroll
        for (int i = 0; i < TPG; ++i) t += p[i] * vfs[i][j];
        acc[h][j] = t;
      }
    }
  };

  {
    uint4 kA[TPG], vA[TPG], kB[TPG], vB[TPG];
    int b = shared_tok / BS + wave;
    if (b < n_blocks) issue_block(bt[b], kA, vA);
    while (b < n_blocks) {
      if (b + 4 < n_blocks) issue_block(bt[b + 4], kB, vB);
      consume_block(b, kA, vA);
      b += 4;
      if (b >= n_blocks) break;
      if (b + 4 < n_blocks) issue_block(bt[b + 4], kA, vA);
      consume_block(b, kB, vB);
      b += 4;
    }
  }

  // ---- in-wave merge of the 4 lane-groups (lanes GW apart hold the same
  //      dims); idle lane-groups (m = kNegInf, l = 0) weigh zero ----
#pragma unroll
  for (int off = GW; off < 64; off <<= 1) {
#pragma unroll
    for (int h = 0; h < GROUP; ++h) {
      const float m_o = __shfl_xor(m[h], off, kWave);
      const float l_o = __shfl_xor(l[h], off, kWave);
      const float M = fmaxf(m[h], m_o);
      const float wa = __expf(m[h] - M);
      const float wb = __expf(m_o - M);
      l[h] = l[h] * wa + l_o * wb;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[h][j] = acc[h][j] * wa + __shfl_xor(acc[h][j], off, kWave) * wb;
      m[h] = M;
    }
  }
  if (group == 0) {
#pragma unroll
    for (int h = 0; h < GROUP; ++h) {
      float* dst = accs + (wave * GROUP + h) * D + d0;
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = acc[h][j];
      if (gl == 0) {
        ml[(wave * GROUP + h) * 2 + 0] = m[h];
        ml[(wave * GROUP + h) * 2 + 1] = l[h];
      }
    }
  }

  // ---- the row's prefix (m, l) of every chunk -> LDS in one parallel
  //      step, so the merge below is a run of independent loads (a chunk
  //      loop that read m, then l, then branched took ~1 us a chunk) ----
  const int64_t pre =
      shared_tok > 0
          ? (int64_t(row_tile[seq]) * n_kv_heads + kvh) * n_chunks * TROWS +
                row_slot[seq] * GROUP
          : 0;
  const int pre_chunks = shared_tok > 0 ? n_chunks : 0;
  for (int idx = threadIdx.x; idx < pre_chunks * GROUP; idx += blockDim.x) {
    const int64_t pr = pre + int64_t(idx / GROUP) * TROWS + idx % GROUP;
    pml[idx * 2 + 0] = ws_ml[pr * 2 + 0];
    pml[idx * 2 + 1] = ws_ml[pr * 2 + 1];
  }
  __syncthreads();

  // ---- final merge: 4 wave partials + the prefix partials; a thread
  //      owns (head, dim) outputs.  An empty chunk is (m = kNegInf,
  //      l = 0, acc = 0) and weighs nothing ----
  for (int idx = threadIdx.x; idx < GROUP * D; idx += blockDim.x) {
    const int h = idx / D;
    const int d = idx % D;
    float M = kNegInf;
    for (int p = 0; p < 4; ++p) M = fmaxf(M, ml[(p * GROUP + h) * 2]);
    for (int c = 0; c < pre_chunks; ++c)
      M = fmaxf(M, pml[(c * GROUP + h) * 2]);
    float num = 0.f, den = 0.f;
    for (int p = 0; p < 4; ++p) {
      const float w = __expf(ml[(p * GROUP + h) * 2] - M);
      num += w * accs[(p * GROUP + h) * D + d];
      den += w * ml[(p * GROUP + h) * 2 + 1];
    }
    const float* pacc = ws_acc + (pre + h) * D + d;
#pragma unroll 8
    for (int c = 0; c < pre_chunks; ++c) {
      const float w = __expf(pml[(c * GROUP + h) * 2] - M);
      num += w * pacc[int64_t(c) * TROWS * D];
      den += w * pml[(c * GROUP + h) * 2 + 1];
    }
    out[(int64_t(seq) * n_kv_heads * GROUP + kvh * GROUP + h) * D + d] =
        f32_to_bf16(den > 0.f ? num / den : 0.f);
  }
}

}  // namespace

// Chunks of the shared prefix per (row tile, kv-head): enough workgroups
// for the 256 CUs, at most one chunk per 64-token KV tile.
int shared_prefix_n_chunks(int tiles, int n_kv_heads, int kv_tiles) {
  const int wgs = tiles * n_kv_heads;
  int n = (256 + wgs - 1) / wgs;
  if (n > kv_tiles) n = kv_tiles;
  if (n > 64) n = 64;
  return n < 1 ? 1 : n;
}

void launch_decode_attn_shared(
    const uint16_t* qkv, const uint16_t* k_cache, const uint16_t* v_cache,
    const int32_t* block_table, const int32_t* seq_lens,
    const int32_t* n_shared, const int32_t* row_tile,
    const int32_t* row_slot, const int32_t* tile_rows,
    const int32_t* tile_blocks, const int32_t* tile_bt_row, float* ws_acc,
    float* ws_ml, uint16_t* out, int batch, int n_tiles, int n_chunks,
    int n_q_heads, int n_kv_heads, int max_blocks, float scale,
    int qkv_stride, hipStream_t stream) {
  if (batch == 0) return;
  auto go = [&](auto group_tag) {
    constexpr int GROUP = decltype(group_tag)::value;
    if (n_tiles > 0)
      hipLaunchKernelGGL(shared_prefix_attn_kernel<GROUP>,
                         dim3(n_tiles, n_kv_heads, n_chunks), dim3(256), 0,
                         stream, qkv, k_cache, v_cache, block_table,
                         tile_rows, tile_blocks, tile_bt_row, ws_acc, ws_ml,
                         n_kv_heads, max_blocks, qkv_stride, scale);
    hipLaunchKernelGGL(shared_suffix_merge_kernel<GROUP>,
                       dim3(batch * n_kv_heads), dim3(256), 0, stream, qkv,
                       k_cache, v_cache, block_table, seq_lens, n_shared,
                       row_tile, row_slot, ws_acc, ws_ml, out, n_kv_heads,
                       max_blocks, n_chunks, scale, qkv_stride);
  };
  if (n_q_heads / n_kv_heads == 4) go(std::integral_constant<int, 4>{});
  else go(std::integral_constant<int, 8>{});
}

}  // namespace rlli
