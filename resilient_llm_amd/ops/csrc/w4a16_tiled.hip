// Tiled W4A16: the int4-weight GEMM of w4a16.hip for 1 <= M <= 256 rows
// (the decode batches past the 64 rows its one-wave kernel takes).  Same
// contract, same packed / s / meta tensors in the same fragment-order
// packing, symmetric and zero-point (ZP) form:
//   out[m,n] = bf16( sum_g f32(s[n,g]) * sum_{k in g} f32(x[m,k]) * q[n,k] )
//   ZP:        ... * (u[n,k] - z[n,g])
//
// Work split.  One workgroup = one 64-column panel x one K-slice of whole
// groups, W = ceil(M / 64) waves; wave w owns rows 64w .. 64w+63 (4 row
// tiles, the accumulator footprint of w4a16_kernel<4, .>).  The panel's
// packed weight crosses HBM once per workgroup: the waves split a group's
// four 1-KiB fragments (and its 64 scales / meta dwords) between them,
// each loads its share nontemporally into a small register ring and
// stores it, still as packed nibbles, into an LDS double buffer.  Every
// wave then reads the whole group back (one conflict-free ds_read_b128
// per column tile at lane * 16), expands the nibbles in registers and
// runs w4a16.hip's group body: 4 granules x (CT + 1) MFMAs per row tile
// into fresh partials - the fifth against -136 (ZP: 1.0) - and the f32
// scale epilogue.  The expansion is repeated by every wave: two VALU ops
// per weight pair, under the MFMAs.  A fragments come straight from
// global memory through the buffer descriptor (no two waves share a row);
// rows at or beyond M bounds-check to zero.
//
// Pipeline, per wave and group i of the slice:
//   read group i from LDS slot i & 1;  store the staged group i + 1 into
//   slot (i + 1) & 1 and refill that register slot with the global load
//   of group i + 1 + D;  MFMAs of group i;  barrier.
// One barrier per group orders both hazards: a slot is overwritten only
// by waves that passed the barrier after its last read, and read only
// after the barrier that follows its stores.  The loads in flight live in
// registers (D groups deep; a wave's share of a group is 16 / W bytes per
// lane, so D grows with W); the LDS side needs two slots only.  Loads past
// the slice are clamped to the last group of K, stored and never read.
//
// Row m depends on row m of x only; the K-slicing (w4a16_tiled_plan) and
// the order of MFMAs into an accumulator depend on (N, K) alone, so a
// row's bits do not depend on M.  No atomics: split-K slices write f32
// slabs [slices, M, N] that w4a16_reduce_kernel sums in slice order.

#include "w4a16_common.h"

namespace rlli {

namespace {

constexpr int LDS_SLOTS = 2;
constexpr int W4_TILED_WORKGROUPS = 256;   // the plan's grid target

template <int W, bool ZP>
__global__ __launch_bounds__(64 * W)
void w4a16_tiled_kernel(const uint16_t* __restrict__ x,
                        const uint32_t* __restrict__ packed,
                        const void* __restrict__ sm,
                        float* __restrict__ out_ws,       // [splitk][M][N]
                        uint16_t* __restrict__ out_bf16,  // [M][N], splitk==1
                        int M, int N, int K, int grp_per_slice, int splitk) {
  constexpr int M_TILES = 4;                 // row tiles per wave
  constexpr int TPW = (CT + W - 1) / W;      // column tiles a wave stages
  constexpr int D = W == 4 ? 4 : (W == 1 ? 1 : 2);   // register ring, groups
  constexpr int U = D > LDS_SLOTS ? D : LDS_SLOTS;   // steady-loop unroll
  static_assert(U % D == 0 && U % LDS_SLOTS == 0);

  __shared__ u32x4 lds_b[LDS_SLOTS][CT][64];   // packed fragments, lane order
  __shared__ unsigned lds_s[LDS_SLOTS][BN];    // scale bits / meta per column

  const int G = K / GROUP;
  const int n_panels = N / BN;
  const int panel = blockIdx.x % n_panels;
  const int slice = blockIdx.x / n_panels;
  const int gbeg = slice * grp_per_slice;
  const int gend = min(gbeg + grp_per_slice, G);   // workgroup-uniform

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int jcol = lane & 15;   // B column / A row (within a 16-tile)
  const int koct = lane >> 4;   // k-octet: 8 contiguous k

  // x rows >= M are hardware-bounds-checked to 0; every packed / scale
  // address is in bounds by construction.
  const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(x), (short)0, M * K * 2, 0x00020000);
  const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(packed), (short)0,
      int(int64_t(N) * K / 2), 0x00020000);
  constexpr int SB = ZP ? 4 : 2;             // bytes per (column, group)
  const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(sm), (short)0, N * G * SB, 0x00020000);

  // this wave's share of a group: column tiles wave, wave + W, ...; the
  // last wave (it never has more tiles than another) also takes the scales
  int voff_b[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
    voff_b[i] = ((panel * CT + min(wave + i * W, CT - 1)) * G * 64 + lane) * 16;
  const int voff_s = (panel * BN + lane) * G * SB;
  const bool stages_s = wave == W - 1;
  int voff_a[M_TILES];
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt)
    voff_a[mt] = ((wave * 64 + mt * 16 + jcol) * K + koct * 8) * 2;

  f32x4 acc[M_TILES][CT];
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int AUX_NT = 2;                  // nontemporal policy
  u32x4 stq[D][TPW];
  unsigned sts[D];
  u32x4 abuf[GRAN][M_TILES];

  auto load_stage = [&](int d, int g) {
    g = min(g, G - 1);                       // SGPR: g is wave-uniform
#pragma unroll
    for (int i = 0; i < TPW; ++i)
      if (wave + i * W < CT)
        stq[d][i] = __builtin_amdgcn_raw_buffer_load_b128(
            wrsrc, voff_b[i], g * 1024, AUX_NT);
    if (stages_s) {
      if constexpr (ZP)
        sts[d] = __builtin_amdgcn_raw_buffer_load_b32(srsrc, voff_s, g * 4, 0);
      else
        sts[d] = __builtin_amdgcn_raw_buffer_load_b16(srsrc, voff_s, g * 2, 0);
    }
  };
  auto store_stage = [&](int d, int slot) {
#pragma unroll
    for (int i = 0; i < TPW; ++i)
      if (wave + i * W < CT) lds_b[slot][wave + i * W][lane] = stq[d][i];
    if (stages_s) lds_s[slot][lane] = sts[d];
  };
  auto load_a = [&](int j, int g) {
    g = min(g, G - 1);
#pragma unroll
    for (int mt = 0; mt < M_TILES; ++mt)
      abuf[j][mt] = __builtin_amdgcn_raw_buffer_load_b128(
          xrsrc, voff_a[mt], (g * GROUP + j * 32) * 2, 0);
  };

  constexpr unsigned FIFTH = ZP ? BF16_ONE : BF16_NEG136;
  const u32x4 neg136 = {FIFTH, FIFTH, FIFTH, FIFTH};   // ZP: ones
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // group i of the slice (i = p mod U): see the pipeline above
  auto step = [&](int p, int g) {
    const int slot = p % LDS_SLOTS;
    u32x4 bq[CT];
    unsigned bs[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      bq[ct] = lds_b[slot][ct][lane];
      bs[ct] = lds_s[slot][ct * 16 + jcol];
    }
    store_stage((p + 1) % D, (p + 1) % LDS_SLOTS);
    load_stage((p + 1) % D, g + 1 + D);

    // one scale group, as w4a16_kernel: 4 granules of [M_TILES x (CT + 1)]
    // MFMAs into fresh partials, then acc += scale * (pacc + sacc), or
    // with a zero-point acc += scale * fma(-(128 + z), sacc, pacc)
    f32x4 pacc[M_TILES][CT];
    f32x4 sacc[M_TILES];
#pragma unroll
    for (int j = 0; j < GRAN; ++j) {
      bf16x8_vec bfrag[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        bfrag[ct] = as_bf16x8(nibbles_to_bf16(bq[ct][j]));
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
      if constexpr (ZP) {
        const float sc = meta_scale(bs[ct]);
        const float nz = meta_negz(bs[ct]);
#pragma unroll
        for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[mt][ct][r] = fmaf(sc, fmaf(nz, sacc[mt][r], pacc[mt][ct][r]),
                                  acc[mt][ct][r]);
      } else {
        const float sc = bf16_to_f32((uint16_t)bs[ct]);
#pragma unroll
        for (int mt = 0; mt < M_TILES; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[mt][ct][r] =
                fmaf(sc, pacc[mt][ct][r] + sacc[mt][r], acc[mt][ct][r]);
      }
    }
    __syncthreads();
    // keep the groups apart, as w4a16_kernel does (register pressure)
    __builtin_amdgcn_sched_barrier(0);
  };

  // prologue: fill the register ring, put the first group into LDS
#pragma unroll
  for (int d = 0; d < D; ++d) load_stage(d, gbeg + d);
#pragma unroll
  for (int j = 0; j < GRAN; ++j) load_a(j, gbeg);
  store_stage(0, 0);
  load_stage(0, gbeg + D);
  __syncthreads();

  int g = gbeg;
  for (; g + U <= gend; g += U) {
#pragma unroll
    for (int p = 0; p < U; ++p) step(p, g + p);
  }
  // tail: < U groups left; the condition is the same for every wave
#pragma unroll
  for (int p = 0; p < U; ++p)
    if (g + p < gend) step(p, g + p);

  // C layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int mt = 0; mt < M_TILES; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int out_row = wave * 64 + mt * 16 + koct * 4 + r;
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

template <bool ZP>
void launch_w4a16_tiled_any(const uint16_t* x, const uint32_t* packed,
                            const void* sm, float* ws, uint16_t* out, int M,
                            int N, int K, int splitk, int grp_per_slice,
                            hipStream_t stream) {
  // one wave per 64 rows that exist: no wave is absent from a barrier
  const int waves = (M + 63) / 64;
  const int blocks = (N / BN) * splitk;
  auto launch = [&](auto w_tag) {
    constexpr int W = decltype(w_tag)::value;
    hipLaunchKernelGGL((w4a16_tiled_kernel<W, ZP>), dim3(blocks),
                       dim3(64 * W), 0, stream, x, packed, sm, ws, out, M, N,
                       K, grp_per_slice, splitk);
  };
  if (waves == 1) launch(std::integral_constant<int, 1>{});
  else if (waves == 2) launch(std::integral_constant<int, 2>{});
  else if (waves == 3) launch(std::integral_constant<int, 3>{});
  else launch(std::integral_constant<int, 4>{});
  if (splitk > 1) {
    const int64_t mn = int64_t(M) * N;
    const int threads = 256;
    const int rblocks = int(std::min<int64_t>((mn + threads - 1) / threads,
                                              2048));
    hipLaunchKernelGGL(w4a16_reduce_kernel, dim3(rblocks), dim3(threads), 0,
                       stream, ws, out, mn, splitk);
  }
}

}  // namespace

void w4a16_tiled_plan(int N, int K, int splitk_req, int* splitk,
                      int* grp_per_slice) {
  const int G = K / GROUP;
  const int panels = N / BN;
  int sk;
  if (splitk_req > 0) {
    sk = std::min(splitk_req, G);
  } else {
    // one workgroup per CU (256 CUs; three or four waves at one wave per
    // SIMD fill a CU), at least 4 groups per slice: the f32 slab costs
    // slices * M * N * 8 bytes of traffic at up to 256 rows
    sk = std::max(1, (W4_TILED_WORKGROUPS + panels - 1) / panels);
    sk = std::min(sk, std::max(1, G / 4));
  }
  const int gps = (G + sk - 1) / sk;
  *grp_per_slice = gps;
  *splitk = (G + gps - 1) / gps;   // no slice without a K range
}

void launch_w4a16_tiled(const uint16_t* x, const uint32_t* packed,
                        const uint16_t* s, float* ws, uint16_t* out, int M,
                        int N, int K, int splitk, int grp_per_slice,
                        hipStream_t stream) {
  launch_w4a16_tiled_any<false>(x, packed, s, ws, out, M, N, K, splitk,
                                grp_per_slice, stream);
}

void launch_w4a16_zp_tiled(const uint16_t* x, const uint32_t* packed,
                           const uint32_t* meta, float* ws, uint16_t* out,
                           int M, int N, int K, int splitk, int grp_per_slice,
                           hipStream_t stream) {
  launch_w4a16_tiled_any<true>(x, packed, meta, ws, out, M, N, K, splitk,
                               grp_per_slice, stream);
}

}  // namespace rlli
