// W4A16: int4 group-quantized weights, bf16 activations.
//
//   w4a16_linear: out[m,n] = bf16( sum_g f32(s[n,g]) * sum_{k in g}
//                                  f32(x[m,k]) * q[n,k] ),   1 <= M <= 64
//   w4_dequant:   w[n,k]   = bf16( f32(s[n,g]) * q[n,k] )
//
// Format (ops/ref.py w4_pack): symmetric, group 128 along K, q in -8..7
// stored as the nibble u = q + 8.  ``packed`` is in MFMA fragment order
// (mfma_f32_16x16x32_bf16: lane l holds 8 contiguous k of column l&15 at
// k-octet l>>4): the dwordx4 at ((tile*G + g)*64 + lane)*16 bytes,
// tile = n/16, holds lane's octet of the four 32-k granules of group g.
// Dword j carries k = g*128 + j*32 + o*8 + i as the nibble at bit
// 4*(i/2) + 16*(i%2), so ``(d >> 4p) & 0x000F000F | 0x43004300`` is the
// bf16 PAIR (128+u) of elements 2p, 2p+1: one shift and one and-or per
// two weights.
//
// The fused GEMM is skinny2.hip's shape: zero LDS, one wave per 64-column
// panel x K-slice, both operands through buffer descriptors, B
// nontemporal.  One 16-byte B load per lane and column tile feeds the 4
// MFMAs of a whole scale group, and a wave's load of one (tile, group) is
// 1 KiB contiguous.  gfx950 has no packed-bf16 VALU, so the offset stays
// in the products: B enters the MFMA as 136 + q, a fifth MFMA per
// (row tile, granule) against the constant -136 accumulates
// -136 * sum_k x[m,k] in the C layout, and the group epilogue is
//     acc += s[n,g] * (pacc + sacc)
// - one add and one FMA per accumulator register per 128 k, no per-weight
// scale multiply.
//
// Row m of the result depends on row m of x only and is bit-identical for
// every M: the K-slicing and the order of MFMAs into an accumulator
// depend on (N, K) alone; the ring depth only moves loads.  No atomics:
// split-K slices write f32 slabs that a second kernel sums in slice
// order.

#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <type_traits>

namespace rlli {

namespace {

using bf16x8_vec = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int BN = 64;          // columns per wave (4 MFMA column tiles)
constexpr int CT = BN / 16;     // column tiles
constexpr int GROUP = 128;      // k per scale group = 4 granules of 32
constexpr int GRAN = GROUP / 32;
constexpr unsigned BF16_128 = 0x43004300u;     // bf16 pair (128, 128)
constexpr unsigned BF16_NEG136 = 0xC308C308u;  // bf16 pair (-136, -136)

DEV_INLINE bf16x8_vec as_bf16x8(u32x4 v) {
  return *reinterpret_cast<bf16x8_vec*>(&v);
}

// 8 nibbles of one dword -> the bf16 fragment (136 + q) of 8 contiguous k
DEV_INLINE u32x4 nibbles_to_bf16(unsigned d) {
  u32x4 f;
  f[0] = (d & 0x000F000Fu) | BF16_128;
  f[1] = ((d >> 4) & 0x000F000Fu) | BF16_128;
  f[2] = ((d >> 8) & 0x000F000Fu) | BF16_128;
  f[3] = ((d >> 12) & 0x000F000Fu) | BF16_128;
  return f;
}

// One wave = one 64-column panel x one K-slice of whole groups.
//  blockIdx.x = panel + n_panels * slice
// GB = depth of the B ring in GROUPS (CT dwordx4 + CT scales each).  The
// A fragments sit in a ring of the 4 granule slots of one group: slot j is
// refilled with the next group's granule j right after its MFMAs, so its
// load has three granules of MFMAs to land.  Loads past the slice are
// issued anyway, clamped to the last group of K (always in bounds), and
// never consumed: the loop body has no load branch.
template <int M_TILES, int GB>
__global__ __launch_bounds__(64)
void w4a16_kernel(const uint16_t* __restrict__ x,
                  const uint32_t* __restrict__ packed,
                  const uint16_t* __restrict__ s,
                  float* __restrict__ out_ws,       // [splitk][M][N] f32
                  uint16_t* __restrict__ out_bf16,  // [M][N] when splitk==1
                  int M, int N, int K, int grp_per_slice, int splitk) {
  const int G = K / GROUP;
  const int n_panels = N / BN;
  const int panel = blockIdx.x % n_panels;
  const int slice = blockIdx.x / n_panels;
  const int gbeg = slice * grp_per_slice;
  const int gend = min(gbeg + grp_per_slice, G);
  if (gbeg >= gend) return;

  const int lane = threadIdx.x;
  const int jcol = lane & 15;   // B column / A row (within a 16-tile)
  const int koct = lane >> 4;   // k-octet: 8 contiguous k

  // x rows >= M are hardware-bounds-checked to 0 (padded M tiles add
  // nothing); every packed / scale address is in bounds by construction.
  const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(x), (short)0, M * K * 2, 0x00020000);
  const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(packed), (short)0,
      int(int64_t(N) * K / 2), 0x00020000);
  const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(s), (short)0, N * G * 2, 0x00020000);

  int voff_b[CT], voff_s[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    voff_b[ct] = ((panel * CT + ct) * G * 64 + lane) * 16;
    voff_s[ct] = (panel * BN + ct * 16 + jcol) * G * 2;
  }
  int voff_a[M_TILES];
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt)
    voff_a[mt] = ((mt * 16 + jcol) * K + koct * 8) * 2;

  f32x4 acc[M_TILES][CT];
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int AUX_NT = 2;                  // nontemporal policy
  u32x4 bq[GB][CT];
  unsigned short bs[GB][CT];
  u32x4 abuf[GRAN][M_TILES];

  auto load_b = [&](int p, int g) {
    g = min(g, G - 1);                       // SGPR: g is wave-uniform
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      bq[p][ct] = __builtin_amdgcn_raw_buffer_load_b128(
          wrsrc, voff_b[ct], g * 1024, AUX_NT);
      bs[p][ct] = __builtin_amdgcn_raw_buffer_load_b16(
          srsrc, voff_s[ct], g * 2, 0);
    }
  };
  auto load_a = [&](int j, int g) {
    g = min(g, G - 1);
#pragma unroll
    for (int mt = 0; mt < M_TILES; ++mt)
      abuf[j][mt] = __builtin_amdgcn_raw_buffer_load_b128(
          xrsrc, voff_a[mt], (g * GROUP + j * 32) * 2, 0);
  };

  const u32x4 neg136 = {BF16_NEG136, BF16_NEG136, BF16_NEG136, BF16_NEG136};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // one scale group: 4 granules of [M_TILES x (CT + 1)] MFMAs into fresh
  // partial accumulators, then acc += scale * (pacc + sacc)
  auto group = [&](int p, int g) {
    f32x4 pacc[M_TILES][CT];
    f32x4 sacc[M_TILES];
#pragma unroll
    for (int j = 0; j < GRAN; ++j) {
      bf16x8_vec bfrag[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        bfrag[ct] = as_bf16x8(nibbles_to_bf16(bq[p][ct][j]));
#pragma unroll
      for (int mt = 0; mt < M_TILES; ++mt) {
        const bf16x8_vec afrag = as_bf16x8(abuf[j][mt]);
        sacc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag, as_bf16x8(neg136), j ? sacc[mt] : zero, 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          pacc[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag, bfrag[ct], j ? pacc[mt][ct] : zero, 0, 0, 0);
      }
      load_a(j, g + 1);
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const float sc = bf16_to_f32(bs[p][ct]);
#pragma unroll
      for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[mt][ct][r] =
              fmaf(sc, pacc[mt][ct][r] + sacc[mt][r], acc[mt][ct][r]);
    }
    // keep the groups apart: interleaving two groups' partial
    // accumulators doubles the live registers (spills at M_TILES = 4)
    __builtin_amdgcn_sched_barrier(0);
  };

  // prologue: fill both rings
#pragma unroll
  for (int p = 0; p < GB; ++p) load_b(p, gbeg + p);
#pragma unroll
  for (int j = 0; j < GRAN; ++j) load_a(j, gbeg);
  // steady: consume group g+p (ring slot p), refill slot p with g+p+GB
  int g = gbeg;
  for (; g + GB <= gend; g += GB) {
#pragma unroll
    for (int p = 0; p < GB; ++p) {
      group(p, g + p);
      load_b(p, g + p + GB);
    }
  }
  // tail: the < GB groups left are already in their slots
#pragma unroll
  for (int p = 0; p < GB; ++p)
    if (g + p < gend) group(p, g + p);

  // C layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int out_row = mt * 16 + koct * 4 + r;
      if (out_row >= M) continue;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int out_col = panel * BN + ct * 16 + jcol;
        if (splitk == 1) {
          out_bf16[int64_t(out_row) * N + out_col] =
              f32_to_bf16(acc[mt][ct][r]);
        } else {
          out_ws[(int64_t(slice) * M + out_row) * N + out_col] =
              acc[mt][ct][r];
        }
      }
    }
  }
}

__global__ void w4a16_reduce_kernel(const float* __restrict__ ws,
                                    uint16_t* __restrict__ out,
                                    int64_t mn, int splitk) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < mn;
       i += stride) {
    float acc = 0.f;
    for (int sl = 0; sl < splitk; ++sl) acc += ws[int64_t(sl) * mn + i];
    out[i] = f32_to_bf16(acc);
  }
}

// One workgroup per (16-row tile, group): thread (c, j, o) turns one dword
// into 8 contiguous bf16 of row tile*16 + c, so 16 threads write one
// 256-byte run of a row.
__global__ __launch_bounds__(256)
void w4_dequant_kernel(const uint32_t* __restrict__ packed,
                       const uint16_t* __restrict__ s,
                       uint16_t* __restrict__ out, int K, bool vec_store) {
  const int G = K / GROUP;
  const int64_t tg = blockIdx.x;             // tile * G + g
  const int g = int(tg % G);
  const int64_t tile = tg / G;
  const int c = threadIdx.x >> 4;
  const int j = (threadIdx.x >> 2) & 3;
  const int o = threadIdx.x & 3;
  const unsigned d = packed[(tg * 64 + o * 16 + c) * 4 + j];
  const int64_t row = tile * 16 + c;
  const float sc = bf16_to_f32(s[row * G + g]);
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int u = (d >> (4 * (i / 2) + 16 * (i % 2))) & 15;
    v.s[i] = f32_to_bf16(sc * float(u - 8));
  }
  uint16_t* dst = out + row * K + g * GROUP + j * 32 + o * 8;
  if (vec_store) {
    *reinterpret_cast<uint4*>(dst) = v.u;
  } else {                      // out not 16-byte aligned (a view)
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = v.s[i];
  }
}

}  // namespace

void w4a16_plan(int N, int K, int splitk_req, int* splitk,
                int* grp_per_slice) {
  const int G = K / GROUP;
  const int panels = N / BN;
  int sk;
  if (splitk_req > 0) {
    sk = std::min(splitk_req, G);
  } else {
    // fill ~1024 waves (4 per CU), but keep >= 4 groups per slice so the
    // ring prologue stays a small part of a wave's life
    sk = std::max(1, (1024 + panels - 1) / panels);
    sk = std::min(sk, std::max(1, G / 4));
  }
  const int gps = (G + sk - 1) / sk;
  *grp_per_slice = gps;
  *splitk = (G + gps - 1) / gps;   // no slice without a K range
}

void launch_w4a16(const uint16_t* x, const uint32_t* packed,
                  const uint16_t* s, float* ws, uint16_t* out, int M, int N,
                  int K, int splitk, int grp_per_slice, hipStream_t stream) {
  const int m_tiles = (M + 15) / 16;
  const int blocks = (N / BN) * splitk;
  auto launch = [&](auto mt_tag, auto gb_tag) {
    hipLaunchKernelGGL((w4a16_kernel<decltype(mt_tag)::value,
                                     decltype(gb_tag)::value>),
                       dim3(blocks), dim3(64), 0, stream, x, packed, s, ws,
                       out, M, N, K, grp_per_slice, splitk);
  };
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using I4 = std::integral_constant<int, 4>;
  // deeper B ring while the accumulators leave room for it
  if (m_tiles == 1) launch(I1{}, I4{});
  else if (m_tiles == 2) launch(I2{}, I3{});
  else if (m_tiles == 3) launch(I3{}, I2{});
  else launch(I4{}, I2{});
  if (splitk > 1) {
    const int64_t mn = int64_t(M) * N;
    const int threads = 256;
    const int rblocks = int(std::min<int64_t>((mn + threads - 1) / threads,
                                              2048));
    hipLaunchKernelGGL(w4a16_reduce_kernel, dim3(rblocks), dim3(threads), 0,
                       stream, ws, out, mn, splitk);
  }
}

void launch_w4_dequant(const uint32_t* packed, const uint16_t* s,
                       uint16_t* out, int N, int K, hipStream_t stream) {
  const int64_t blocks = int64_t(N / 16) * (K / GROUP);
  const bool vec_store = reinterpret_cast<uintptr_t>(out) % 16 == 0;
  hipLaunchKernelGGL(w4_dequant_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     stream, packed, s, out, K, vec_store);
}

}  // namespace rlli
