// Wide W4A16: the int4-weight GEMM of w4a16.hip for 1 <= M <= 512 rows
// (mixed chunked-prefill steps past the 256 rows w4a16_tiled.hip takes).
// Same contract, same packed / s / meta tensors, symmetric and zero-point
// (ZP) form:
//   out[m,n] = bf16( sum_g f32(s[n,g]) * sum_{k in g} f32(x[m,k]) * q[n,k] )
//   ZP:        ... * (u[n,k] - z[n,g])
//
// Work split.  One workgroup = one 128-column panel x one block of 128
// rows x one K-slice of whole groups, always four waves; wave w owns rows
// 32w .. 32w+31 of the block: 2 row tiles x 8 column tiles, the 16
// accumulator tiles per wave of the tiled kernel, so a running and a
// partial accumulator set (128 registers) fit.  blockIdx.x = row block +
// row_blocks * (panel + panels * slice): the workgroups that read the same
// weight are neighbours in launch order.  A panel's rows of x are read
// once per 128 columns, half the tiled kernel's traffic.
//
// Weights are converted once per workgroup, on the way into LDS.  Each
// thread loads two 16-byte packed fragments of a group nontemporally
// (column tiles w and w + 4) into a register ring two groups deep, expands
// every dword into the bf16 MFMA B fragment of 8 contiguous k and stores
// 16 bytes at [tile][granule][lane]: a 128 x 128 group is 32 KiB of bf16,
// double-buffered.  A wave's B operand is then one conflict-free
// ds_read_b128, with no VALU work behind it.  The bf16 holds the nibble
// with an offset that one integer operation per PAIR of weights puts
// there, exactly:
//   symmetric   0x4300 | u           = bf16(128 + u)     = 136 + q
//   zero-point  (0x4310 - z) + u     = bf16(144 + u - z)   (129 .. 159)
// so the zero-point leaves the epilogue.  The offset comes out through
// one MFMA per (row tile, granule) against the constant -136 / -144 -
// 8 of 72 MFMAs per wave and group, where the tiled kernel pays 16 of 80 -
// whose result seeds the group's partial accumulators as their C operand:
// the partial ends as sum_k x * (u - z), and the group epilogue is the one
// FMA  acc += s[n,g] * pacc  per accumulator register, for both forms.
// (A true bf16(u - z) in LDS would delete those 8 MFMAs and cost about
// three VALU operations per weight to build; profiles/w4a16_wide.md counts
// both.)  A fragments come straight from global memory through the buffer
// descriptor into a register double buffer, two groups ahead: the seed
// MFMAs need all four granules of a group at its start, and loads return
// in order, so a weight load is waited for as soon as a younger A load
// is.  Rows at or beyond M bounds-check to zero.
//
// Pipeline per group i of the slice, as in the tiled kernel: convert and
// store the staged group i + 1 into LDS slot (i + 1) & 1, refill that
// register slot with the global load of group i + 1 + RING, MFMAs of group
// i from slot i & 1 (granule j's A registers are refilled with group
// i + 2 right after its MFMAs), barrier.  Loads past the slice are clamped to the last
// group of K, stored and never read.
//
// Row m depends on row m of x only; the K-slicing (w4a16_wide_plan) and
// the order of MFMAs into an accumulator depend on (N, K) alone, so a
// row's bits do not depend on M.  No atomics: split-K slices write f32
// slabs [slices, M, N] that w4a16_reduce_kernel sums in slice order.

#include "w4a16_common.h"

namespace rlli {

namespace {

constexpr int WN = 128;                    // columns per workgroup
constexpr int WCT = WN / 16;               // column tiles
constexpr int WM = 128;                    // rows per workgroup
constexpr int WAVES = 4;
constexpr int WMT = WM / WAVES / 16;       // row tiles per wave
constexpr int TPW = WCT / WAVES;           // column tiles a wave stages
constexpr int RING = 2;                    // register ring, groups
constexpr int LDS_SLOTS = 2;
constexpr int A_SLOTS = 2;                 // A fragments in registers, groups
constexpr int W4_WIDE_PANEL_SLICES = 128;  // the plan's (panel, slice) target
constexpr unsigned BF16_NEG144 = 0xC310C310u;   // bf16 pair (-144, -144)
static_assert(RING % LDS_SLOTS == 0 && RING % A_SLOTS == 0);

// 8 nibbles of one dword -> the bf16 fragment (144 + u - z) of 8
// contiguous k; c = (0x4310 - z) in both halves, no carry between them
DEV_INLINE u32x4 nibbles_to_bf16_zp(unsigned d, unsigned c) {
  u32x4 f;
  f[0] = (d & 0x000F000Fu) + c;
  f[1] = ((d >> 4) & 0x000F000Fu) + c;
  f[2] = ((d >> 8) & 0x000F000Fu) + c;
  f[3] = ((d >> 12) & 0x000F000Fu) + c;
  return f;
}

template <bool ZP>
__global__ __launch_bounds__(64 * WAVES)
void w4a16_wide_kernel(const uint16_t* __restrict__ x,
                       const uint32_t* __restrict__ packed,
                       const void* __restrict__ sm,
                       float* __restrict__ out_ws,       // [splitk][M][N]
                       uint16_t* __restrict__ out_bf16,  // [M][N], splitk==1
                       int M, int N, int K, int grp_per_slice, int splitk,
                       int row_blocks) {
  // bf16 B fragments of one group per slot, [tile][granule][lane]
  __shared__ u32x4 lds_b[LDS_SLOTS][WCT][GRAN][64];
  __shared__ unsigned lds_s[LDS_SLOTS][WN];   // scale bits / meta per column

  const int G = K / GROUP;
  const int n_panels = N / WN;
  const int rblk = blockIdx.x % row_blocks;
  const int ps = blockIdx.x / row_blocks;
  const int panel = ps % n_panels;
  const int slice = ps / n_panels;
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

  // this thread's share of a group: its lane's 16 bytes of column tiles
  // wave and wave + 4, and those columns' scale / meta
  int voff_b[TPW], voff_s[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int ct = wave + i * WAVES;
    voff_b[i] = ((panel * WCT + ct) * G * 64 + lane) * 16;
    voff_s[i] = (panel * WN + ct * 16 + jcol) * G * SB;
  }
  const int row0 = rblk * WM + wave * (16 * WMT);
  int voff_a[WMT];
#pragma unroll
  for (int mt = 0; mt < WMT; ++mt)
    voff_a[mt] = ((row0 + mt * 16 + jcol) * K + koct * 8) * 2;

  f32x4 acc[WMT][WCT];
#pragma unroll
  for (int mt = 0; mt < WMT; ++mt)
#pragma unroll
    for (int ct = 0; ct < WCT; ++ct) acc[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int AUX_NT = 2;                  // nontemporal policy
  u32x4 stq[RING][TPW];
  unsigned sts[RING][TPW];
  u32x4 abuf[A_SLOTS][GRAN][WMT];

  auto load_stage = [&](int d, int g) {
    g = min(g, G - 1);                       // SGPR: g is wave-uniform
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      stq[d][i] = __builtin_amdgcn_raw_buffer_load_b128(
          wrsrc, voff_b[i], g * 1024, AUX_NT);
      if constexpr (ZP)
        sts[d][i] = __builtin_amdgcn_raw_buffer_load_b32(
            srsrc, voff_s[i], g * 4, 0);
      else
        sts[d][i] = __builtin_amdgcn_raw_buffer_load_b16(
            srsrc, voff_s[i], g * 2, 0);
    }
  };
  auto store_stage = [&](int d, int slot) {
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int ct = wave + i * WAVES;
#pragma unroll
      for (int j = 0; j < GRAN; ++j) {
        if constexpr (ZP) {
          // meta's high half is bf16(-(128 + z)) = 0xC300 | z
          const unsigned z = (sts[d][i] >> 16) & 15u;
          lds_b[slot][ct][j][lane] =
              nibbles_to_bf16_zp(stq[d][i][j], (0x4310u - z) * 0x00010001u);
        } else {
          lds_b[slot][ct][j][lane] = nibbles_to_bf16(stq[d][i][j]);
        }
      }
      if (koct == 0) lds_s[slot][ct * 16 + jcol] = sts[d][i];
    }
  };
  auto load_a = [&](int a, int j, int g) {
    g = min(g, G - 1);
#pragma unroll
    for (int mt = 0; mt < WMT; ++mt)
      abuf[a][j][mt] = __builtin_amdgcn_raw_buffer_load_b128(
          xrsrc, voff_a[mt], (g * GROUP + j * 32) * 2, 0);
  };

  constexpr unsigned OFFSET = ZP ? BF16_NEG144 : BF16_NEG136;
  const u32x4 offset = {OFFSET, OFFSET, OFFSET, OFFSET};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // group i of the slice (i = p mod RING): see the pipeline above
  auto step = [&](int p, int g) {
    const int slot = p % LDS_SLOTS;
    const int a = p % A_SLOTS;
    unsigned bs[WCT];
#pragma unroll
    for (int ct = 0; ct < WCT; ++ct) bs[ct] = lds_s[slot][ct * 16 + jcol];
    store_stage((p + 1) % RING, (p + 1) % LDS_SLOTS);
    load_stage((p + 1) % RING, g + 1 + RING);

    // -offset * sum_k x[m,k] of the group, in the C layout of every
    // column tile: the seed of the partial accumulators
    f32x4 seed[WMT];
#pragma unroll
    for (int j = 0; j < GRAN; ++j)
#pragma unroll
      for (int mt = 0; mt < WMT; ++mt)
        seed[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            as_bf16x8(abuf[a][j][mt]), as_bf16x8(offset), j ? seed[mt] : zero,
            0, 0, 0);
    f32x4 pacc[WMT][WCT];
#pragma unroll
    for (int j = 0; j < GRAN; ++j) {
      bf16x8_vec bfrag[WCT];
#pragma unroll
      for (int ct = 0; ct < WCT; ++ct)
        bfrag[ct] = as_bf16x8(lds_b[slot][ct][j][lane]);
#pragma unroll
      for (int mt = 0; mt < WMT; ++mt) {
        const bf16x8_vec afrag = as_bf16x8(abuf[a][j][mt]);
#pragma unroll
        for (int ct = 0; ct < WCT; ++ct)
          pacc[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag, bfrag[ct], j ? pacc[mt][ct] : seed[mt], 0, 0, 0);
      }
      load_a(a, j, g + A_SLOTS);
    }
#pragma unroll
    for (int ct = 0; ct < WCT; ++ct) {
      const float sc = ZP ? meta_scale(bs[ct])
                          : bf16_to_f32((uint16_t)bs[ct]);
#pragma unroll
      for (int mt = 0; mt < WMT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[mt][ct][r] = fmaf(sc, pacc[mt][ct][r], acc[mt][ct][r]);
    }
    __syncthreads();
    // keep the groups apart, as w4a16_kernel does (register pressure)
    __builtin_amdgcn_sched_barrier(0);
  };

  // prologue: fill the register ring, put the first group into LDS
#pragma unroll
  for (int d = 0; d < RING; ++d) load_stage(d, gbeg + d);
#pragma unroll
  for (int a = 0; a < A_SLOTS; ++a)
#pragma unroll
    for (int j = 0; j < GRAN; ++j) load_a(a, j, gbeg + a);
  store_stage(0, 0);
  load_stage(0, gbeg + RING);
  __syncthreads();

  int g = gbeg;
  for (; g + RING <= gend; g += RING) {
#pragma unroll
    for (int p = 0; p < RING; ++p) step(p, g + p);
  }
  // tail: < RING groups left; the condition is the same for every wave
#pragma unroll
  for (int p = 0; p < RING; ++p)
    if (g + p < gend) step(p, g + p);

  // C layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int mt = 0; mt < WMT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int out_row = row0 + mt * 16 + koct * 4 + r;
      if (out_row >= M) continue;
#pragma unroll
      for (int ct = 0; ct < WCT; ++ct) {
        const int out_col = panel * WN + ct * 16 + jcol;
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
void launch_w4a16_wide_any(const uint16_t* x, const uint32_t* packed,
                           const void* sm, float* ws, uint16_t* out, int M,
                           int N, int K, int splitk, int grp_per_slice,
                           hipStream_t stream) {
  const int row_blocks = (M + WM - 1) / WM;
  const int blocks = (N / WN) * splitk * row_blocks;
  hipLaunchKernelGGL(w4a16_wide_kernel<ZP>, dim3(blocks), dim3(64 * WAVES),
                     0, stream, x, packed, sm, ws, out, M, N, K,
                     grp_per_slice, splitk, row_blocks);
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

void w4a16_wide_plan(int N, int K, int splitk_req, int* splitk,
                     int* grp_per_slice) {
  const int G = K / GROUP;
  const int panels = N / WN;
  int sk;
  if (splitk_req > 0) {
    sk = std::min(splitk_req, G);
  } else {
    // 128 (panel, slice) pairs: with the 2 .. 4 row blocks of 129 .. 512
    // rows that is one or two workgroups per CU; at least 4 groups per
    // slice, and no more slices than that, because the f32 slab costs
    // slices * M * N * 8 bytes of traffic at up to 512 rows
    sk = std::max(1, (W4_WIDE_PANEL_SLICES + panels - 1) / panels);
    sk = std::min(sk, std::max(1, G / 4));
  }
  const int gps = (G + sk - 1) / sk;
  *grp_per_slice = gps;
  *splitk = (G + gps - 1) / gps;   // no slice without a K range
}

void launch_w4a16_wide(const uint16_t* x, const uint32_t* packed,
                       const uint16_t* s, float* ws, uint16_t* out, int M,
                       int N, int K, int splitk, int grp_per_slice,
                       hipStream_t stream) {
  launch_w4a16_wide_any<false>(x, packed, s, ws, out, M, N, K, splitk,
                               grp_per_slice, stream);
}

void launch_w4a16_zp_wide(const uint16_t* x, const uint32_t* packed,
                          const uint32_t* meta, float* ws, uint16_t* out,
                          int M, int N, int K, int splitk, int grp_per_slice,
                          hipStream_t stream) {
  launch_w4a16_wide_any<true>(x, packed, meta, ws, out, M, N, K, splitk,
                              grp_per_slice, stream);
}

}  // namespace rlli
