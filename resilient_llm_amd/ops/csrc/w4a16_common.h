// Shared by w4a16.hip (symmetric) and w4a16_zp.hip (zero-point): the
// kernel templates and their launchers.  See w4a16.hip for the format
// and the design.
#pragma once

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
constexpr unsigned BF16_ONE = 0x3F803F80u;     // bf16 pair (1, 1)

DEV_INLINE float f16_to_f32(unsigned short h) {
  return float(*reinterpret_cast<const _Float16*>(&h));
}
// meta dword -> (scale, -(128 + z))
DEV_INLINE float meta_scale(unsigned m) { return f16_to_f32((unsigned short)m); }
DEV_INLINE float meta_negz(unsigned m) {
  return __builtin_bit_cast(float, m & 0xFFFF0000u);
}

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

// 8 (gate, up) bf16 pairs of one lane -> the A fragment of their SwiGLU
DEV_INLINE u32x4 silu_mul_frag(u32x4 g, u32x4 u) {
  u32x4 a;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const unsigned lo = silu_mul_bf16(uint16_t(g[p]), uint16_t(u[p]));
    const unsigned hi = silu_mul_bf16(uint16_t(g[p] >> 16),
                                      uint16_t(u[p] >> 16));
    a[p] = lo | (hi << 16);
  }
  return a;
}

// One wave = one 64-column panel x one K-slice of whole groups.
//  blockIdx.x = panel + n_panels * slice
// GB = depth of the B ring in GROUPS (CT dwordx4 + CT scales each).  The
// A fragments sit in a ring of the 4 granule slots of one group: slot j is
// refilled with the next group's granule j right after its MFMAs, so its
// load has three granules of MFMAs to land.  Loads past the slice are
// issued anyway, clamped to the last group of K (always in bounds), and
// never consumed: the loop body has no load branch.
// ZP: ``sm`` is meta u32 [N, G] instead of the bf16 scales [N, G].
// SILU (w4a16_silu.hip): ``x`` is gu [M, 2K], the packed gate|up rows, and
// the A fragment is bf16(silu(g) * u).  Every ring slot then holds the
// gate and the up octet (two loads where the plain form issues one, at
// the same distance ahead) and the activation is computed on the slot's
// registers right before the MFMAs that consume it; everything after the
// A fragment is the plain kernel.
template <int M_TILES, int GB, bool ZP, bool SILU = false>
__global__ __launch_bounds__(64)
void w4a16_kernel(const uint16_t* __restrict__ x,
                  const uint32_t* __restrict__ packed,
                  const void* __restrict__ sm,
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
  // nothing: silu(0) * 0 = 0 too); every packed / scale address is in
  // bounds by construction.
  constexpr int AV = SILU ? 2 : 1;           // operands per A fragment
  const int lda = AV * K;                    // row stride of x / gu
  const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(x), (short)0, M * lda * 2, 0x00020000);
  const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(packed), (short)0,
      int(int64_t(N) * K / 2), 0x00020000);
  constexpr int SB = ZP ? 4 : 2;             // bytes per (column, group)
  const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(sm), (short)0, N * G * SB, 0x00020000);

  int voff_b[CT], voff_s[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    voff_b[ct] = ((panel * CT + ct) * G * 64 + lane) * 16;
    voff_s[ct] = (panel * BN + ct * 16 + jcol) * G * SB;
  }
  int voff_a[M_TILES];
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt)
    voff_a[mt] = ((mt * 16 + jcol) * lda + koct * 8) * 2;

  f32x4 acc[M_TILES][CT];
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int AUX_NT = 2;                  // nontemporal policy
  u32x4 bq[GB][CT];
  std::conditional_t<ZP, unsigned, unsigned short> bs[GB][CT];
  u32x4 abuf[GRAN][M_TILES][AV];             // SILU: [0] gate, [1] up

  auto load_b = [&](int p, int g) {
    g = min(g, G - 1);                       // SGPR: g is wave-uniform
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      bq[p][ct] = __builtin_amdgcn_raw_buffer_load_b128(
          wrsrc, voff_b[ct], g * 1024, AUX_NT);
      if constexpr (ZP)
        bs[p][ct] = __builtin_amdgcn_raw_buffer_load_b32(
            srsrc, voff_s[ct], g * 4, 0);
      else
        bs[p][ct] = __builtin_amdgcn_raw_buffer_load_b16(
            srsrc, voff_s[ct], g * 2, 0);
    }
  };
  auto load_a = [&](int j, int g) {
    g = min(g, G - 1);
#pragma unroll
    for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
      for (int v = 0; v < AV; ++v)
        abuf[j][mt][v] = __builtin_amdgcn_raw_buffer_load_b128(
            xrsrc, voff_a[mt], (v * K + g * GROUP + j * 32) * 2, 0);
  };

  constexpr unsigned FIFTH = ZP ? BF16_ONE : BF16_NEG136;
  const u32x4 neg136 = {FIFTH, FIFTH, FIFTH, FIFTH};   // ZP: ones
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // one scale group: 4 granules of [M_TILES x (CT + 1)] MFMAs into fresh
  // partial accumulators, then acc += scale * (pacc + sacc), or with a
  // zero-point acc += scale * fma(-(128 + z), sacc, pacc)
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
        bf16x8_vec afrag;
        if constexpr (SILU)
          afrag = as_bf16x8(silu_mul_frag(abuf[j][mt][0], abuf[j][mt][1]));
        else
          afrag = as_bf16x8(abuf[j][mt][0]);
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
      if constexpr (ZP) {
        const float sc = meta_scale(bs[p][ct]);
        const float nz = meta_negz(bs[p][ct]);
#pragma unroll
        for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[mt][ct][r] = fmaf(sc, fmaf(nz, sacc[mt][r], pacc[mt][ct][r]),
                                  acc[mt][ct][r]);
      } else {
        const float sc = bf16_to_f32(bs[p][ct]);
#pragma unroll
        for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[mt][ct][r] =
                fmaf(sc, pacc[mt][ct][r] + sacc[mt][r], acc[mt][ct][r]);
      }
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
template <bool ZP>
__global__ __launch_bounds__(256)
void w4_dequant_kernel(const uint32_t* __restrict__ packed,
                       const void* __restrict__ sm,   // s, or (ZP) meta
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
  float sc;
  int z = 8;
  if constexpr (ZP) {
    const unsigned m = static_cast<const uint32_t*>(sm)[row * G + g];
    sc = meta_scale(m);
    z = (m >> 16) & 15;
  } else {
    sc = bf16_to_f32(static_cast<const uint16_t*>(sm)[row * G + g]);
  }
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int u = (d >> (4 * (i / 2) + 16 * (i % 2))) & 15;
    v.s[i] = f32_to_bf16(sc * float(u - z));
  }
  uint16_t* dst = out + row * K + g * GROUP + j * 32 + o * 8;
  if (vec_store) {
    *reinterpret_cast<uint4*>(dst) = v.u;
  } else {                      // out not 16-byte aligned (a view)
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = v.s[i];
  }
}

template <bool ZP, bool SILU = false>
void launch_w4a16_any(const uint16_t* x, const uint32_t* packed,
                      const void* sm, float* ws, uint16_t* out, int M, int N,
                      int K, int splitk, int grp_per_slice,
                      hipStream_t stream) {
  const int m_tiles = (M + 15) / 16;
  const int blocks = (N / BN) * splitk;
  auto launch = [&](auto mt_tag, auto gb_tag) {
    hipLaunchKernelGGL((w4a16_kernel<decltype(mt_tag)::value,
                                     decltype(gb_tag)::value, ZP, SILU>),
                       dim3(blocks), dim3(64), 0, stream, x, packed, sm, ws,
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

template <bool ZP>
void launch_w4_dequant_any(const uint32_t* packed, const void* sm,
                           uint16_t* out, int N, int K, hipStream_t stream) {
  const int64_t blocks = int64_t(N / 16) * (K / GROUP);
  const bool vec_store = reinterpret_cast<uintptr_t>(out) % 16 == 0;
  hipLaunchKernelGGL(w4_dequant_kernel<ZP>, dim3((unsigned)blocks), dim3(256),
                     0, stream, packed, sm, out, K, vec_store);
}

}  // namespace

}  // namespace rlli
