// Mixture-of-Experts MLP (Qwen3-MoE): top-k router, expert alignment,
// grouped gate/up GEMM with SwiGLU in the epilogue, grouped down GEMM and
// a deterministic combine.  bf16 weights, f32 accumulation, one GPU.
// Everything runs on the device: no grid depends on device data and
// nothing is read back, so the four launches of launch_moe_mlp replay
// inside the captured decode graph.
//
// route   one wave per token, 4 tokens per workgroup.  Lane l holds the
//         logits of experts l, l+64, l+128, l+192 (E <= 256).  Selection
//         runs on the logit VALUES: each one becomes a 64-bit key
//         (order-preserving bits of the f32, then 255 - index), so k rounds
//         of a wave-wide max give the k largest in descending order with
//         ties to the lower index.  NaN sorts as -inf and -0 as +0, which
//         is what a stable descending sort of ref.moe_route sees.  A key is
//         never 0 for a real expert, so a row of NaN/Inf still yields k
//         distinct ids below E.  Weights: f32 softmax over all E at the
//         chosen ids, optionally divided by their sum in slot order.
//
// align   one workgroup per expert.  Each counts ALL pairs into an LDS
//         histogram (integer LDS atomics: the counts are exact whatever
//         the order), turns it into whole row tiles of R rows per expert,
//         and takes its own tile offset as the sum of the tiles of the
//         experts before it.  It then walks the pairs once more in order,
//         256 at a time, and places its own by ballot + prefix popcount:
//         within an expert the rows ascend by (token, slot).  The tail of
//         its last tile is marked -1.  Expert 0 also writes the live tile
//         count and pos = -1 for ids outside [0, E), which are then
//         dropped by the combine.  The GEMM grids use the closed-form
//         worst case  tiles <= floor((P + min(E, P) * (R - 1)) / R),
//         P = T * k  (every non-empty expert wastes at most R - 1 rows);
//         tiles at or past the live count exit at once.
//         R = 16 while T * k < 16 * E (a mean of under 16 rows per expert:
//         decode), else 64.
//
// gemm    one workgroup of 4 waves per (row tile, column panel).  The four
//         waves split K between them in 32-k granules (wave w takes
//         granules w, w + 4, ...: together they read each weight row as
//         one contiguous 256 B run), each accumulates the whole tile in
//         registers, waves 1-3 hand their partial sums to wave 0 through
//         LDS and wave 0 runs the epilogue.  The sum order (0, 1, 2, 3) is
//         fixed, so two runs give the same bits.  K-split INSIDE the
//         workgroup is what lets SwiGLU sit in the gate/up epilogue: no
//         partial sum ever leaves the workgroup before the nonlinearity.
//         Operands load straight from memory in mfma_f32_16x16x32_bf16
//         fragment order, as skinny2 does (lane l: 8 contiguous k of
//         row/col l & 15 at k-octet l >> 4):
//           A  gate/up: row tok(p) of x gathered through the sorted index;
//              down: row p of act.  Pad rows (-1) load nothing (a zero
//              fragment) and store nothing.
//           B  16 B of one weight row of the tile's expert, nontemporal
//              (read once); experts no tile names are never touched.
//         A register ring of G granules per wave keeps G - 1 granules of
//         loads in flight behind the MFMAs.
//         Panels:  R = 16: gate/up 16 act columns (16 gate + 16 up rows of
//                  W, NB = 2 B fragments per granule), down 32 columns,
//                  ring depth 8;
//                  R = 64: gate/up 32 act columns (NB = 4), down 64
//                  columns, ring depth 4 (8 fragments per granule).
//         The gate/up workgroup holds the gate and the up accumulator of
//         the same columns, keeps both in f32 and rounds once:
//         act = bf16(silu(g) * u).  The down GEMM writes f32 rows y[p].
//
// Filling 256 CUs at decode: T = 1 at the 30B-A3B layer (H 2048, I 768,
// k 8) has 8 live tiles.  gate/up: 8 tiles x 48 panels = 384 workgroups =
// 1536 waves, each streaming 32 weight rows x 512 k (32 KB); down: 8 x 64
// panels = 512 workgroups = 2048 waves of 32 rows x 192 k.  So the narrow
// panels plus the 4-way K-split give 6-8 waves per CU with 8 tiles; wider
// panels would reuse A more but A is one L2-resident row here.
//
// combine one workgroup per token: out[t] = bf16(sum_j w[t,j] * y[pos(t,j)])
//         in slot order j = 0..k-1, f32.  No atomics anywhere on floats.

#include "common.h"
#include "kernels.h"

#include <cmath>

namespace rlli {

namespace {

using bf16x8_vec = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

DEV_INLINE bf16x8_vec as_bf16x8(u32x4 v) {
  return *reinterpret_cast<bf16x8_vec*>(&v);
}

DEV_INLINE int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

DEV_INLINE unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, kWave);
    v = o > v ? o : v;
  }
  return v;
}

// ------------------------------------------------------------------ route
constexpr int kRouteWaves = 4;

__global__ __launch_bounds__(kRouteWaves * 64)
void moe_route_kernel(const uint16_t* __restrict__ logits,
                      int32_t* __restrict__ ids, float* __restrict__ wts,
                      int T, int E, int k, int renorm) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * kRouteWaves + (threadIdx.x >> 6);
  if (t >= T) return;                       // wave-uniform
  const uint16_t* row = logits + int64_t(t) * E;

  float v[4];
  unsigned long long key[4];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + 64 * i;
    v[i] = -INFINITY;
    key[i] = 0ull;                          // no expert here: never chosen
    if (e < E) {
      v[i] = bf16_to_f32(row[e]);
      float s = v[i];
      if (s != s) s = -INFINITY;            // NaN: the lowest value
      if (s == 0.f) s = 0.f;                // -0 ties with +0
      const uint32_t u = __float_as_uint(s);
      const uint32_t ord = (u >> 31) ? ~u : (u | 0x80000000u);
      key[i] = ((static_cast<unsigned long long>(ord) + 1ull) << 8) |
               static_cast<unsigned long long>(255 - e);
      m = fmaxf(m, v[i]);
    }
  }
  m = wave_max(m);
  float ex[4];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ex[i] = (lane + 64 * i < E) ? expf(v[i] - m) : 0.f;
    sum += ex[i];
  }
  sum = wave_sum(sum);
  const float inv = 1.f / sum;

  int my_id = 0;
  float my_p = 0.f;
  float chosen = 0.f;                       // sum of chosen p, slot order
  for (int j = 0; j < k; ++j) {
    unsigned long long best = key[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) best = key[i] > best ? key[i] : best;
    best = wave_max_u64(best);
    const int e_sel = 255 - int(best & 255ull);
    const int slot = e_sel >> 6;
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i == slot) {
        mine = ex[i];
        if (lane == (e_sel & 63)) key[i] = 0ull;   // taken
      }
    }
    const float p = __shfl(mine, e_sel & 63, kWave) * inv;
    chosen += p;
    if (lane == j) {
      my_id = e_sel;
      my_p = p;
    }
  }
  if (lane < k) {
    ids[int64_t(t) * k + lane] = my_id;
    wts[int64_t(t) * k + lane] = renorm ? my_p / chosen : my_p;
  }
}

// ------------------------------------------------------------------ align
__global__ __launch_bounds__(256)
void moe_align_kernel(const int32_t* __restrict__ ids, int P, int E, int R,
                      int32_t* __restrict__ sorted,
                      int32_t* __restrict__ tile_expert,
                      int32_t* __restrict__ pos,
                      int32_t* __restrict__ n_live) {
  __shared__ int cnt[256];
  __shared__ int wcnt[2][4];
  __shared__ int s_off, s_total;
  const int e = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  cnt[tid] = 0;
  if (tid == 0) {
    s_off = 0;
    s_total = 0;
  }
  __syncthreads();
  for (int i = tid; i < P; i += 256) {
    const int id = ids[i];
    if (unsigned(id) < unsigned(E)) atomicAdd(&cnt[id], 1);
    else if (e == 0) pos[i] = -1;           // dropped by the combine
  }
  __syncthreads();
  {
    const int tiles = tid < E ? (cnt[tid] + R - 1) / R : 0;
    const int before = wave_sum_int(tid < e ? tiles : 0);
    const int total = wave_sum_int(tiles);
    if (lane == 0) {
      atomicAdd(&s_off, before);
      atomicAdd(&s_total, total);
    }
  }
  __syncthreads();
  const int my_cnt = cnt[e];
  const int my_tiles = (my_cnt + R - 1) / R;
  const int tile0 = s_off;
  const int base = tile0 * R;
  if (e == 0 && tid == 0) *n_live = s_total;
  if (my_cnt == 0) return;                  // uniform: no tile, no row
  for (int i = tid; i < my_tiles; i += 256) tile_expert[tile0 + i] = e;
  for (int i = my_cnt + tid; i < my_tiles * R; i += 256) sorted[base + i] = -1;

  int running = 0;
  for (int b = 0, it = 0; b < P && running < my_cnt; b += 256, ++it) {
    const int i = b + tid;
    const bool match = i < P && ids[i] == e;
    const unsigned long long bal = __ballot(match);
    const int buf = it & 1;
    if (lane == 0) wcnt[buf][wave] = __popcll(bal);
    __syncthreads();
    int pre = running, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wcnt[buf][w];
      if (w < wave) pre += c;
      tot += c;
    }
    if (match) {
      const int r = pre + __popcll(bal & ((1ull << lane) - 1ull));
      sorted[base + r] = i;
      pos[i] = base + r;
    }
    running += tot;
  }
}

// ------------------------------------------------------------------- gemm
enum { MODE_GU = 0, MODE_DOWN = 1 };

// MT: 16-row M tiles per row tile (R = 16 * MT).  NB: B fragments per
// granule: MODE_GU NB/2 gate + NB/2 up column tiles (panel = 8 * NB act
// columns), MODE_DOWN NB column tiles (panel = 16 * NB).  G: ring depth.
//   blockIdx.x = tile * n_panels + panel
// N: output columns (I for gate/up, H for down); K: reduction length.
template <int MT, int NB, int MODE, int G>
__global__ __launch_bounds__(256)
void moe_gemm_kernel(const uint16_t* __restrict__ a,
                     const uint16_t* __restrict__ w,
                     const int32_t* __restrict__ sorted,
                     const int32_t* __restrict__ tile_expert,
                     const int32_t* __restrict__ n_live,
                     uint16_t* __restrict__ act_out,
                     float* __restrict__ y_out, int N, int K, int topk) {
  constexpr int R = MT * 16;
  constexpr int PANEL = MODE == MODE_GU ? NB * 8 : NB * 16;
  constexpr int HALF = NB / 2;
  __shared__ f32x4 red[3][MT * NB][64];

  const int n_panels = N / PANEL;
  const int tile = blockIdx.x / n_panels;
  const int panel = blockIdx.x % n_panels;
  if (tile >= *n_live) return;              // uniform
  const int e = tile_expert[tile];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int jcol = lane & 15;
  const int koct = lane >> 4;
  const u32x4 zero = u32x4{0u, 0u, 0u, 0u};

  const uint16_t* a_ptr[MT];
  bool a_ok[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = tile * R + mt * 16 + jcol;
    const int sp = sorted[p];
    a_ok[mt] = sp >= 0;
    const int arow = MODE == MODE_GU ? sp / topk : p;
    a_ptr[mt] = a + int64_t(a_ok[mt] ? arow : 0) * K + koct * 8;
  }
  const uint16_t* b_ptr[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    int64_t wrow;
    if (MODE == MODE_GU)
      wrow = int64_t(e) * 2 * N + (nb / HALF) * N + panel * PANEL +
             (nb % HALF) * 16 + jcol;
    else
      wrow = int64_t(e) * N + panel * PANEL + nb * 16 + jcol;
    b_ptr[nb] = w + wrow * K + koct * 8;
  }

  f32x4 acc[MT][NB];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mt][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 bbuf[G][NB];
  u32x4 abuf[G][MT];
  // this wave's granules: wave, wave + 4, ... below K / 32
  const int n_all = K / 32;
  const int n_g = n_all > wave ? (n_all - wave + 3) / 4 : 0;

  auto load_gran = [&](int p, int g) {
    const int kk = (wave + 4 * g) * 32;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      bbuf[p][nb] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(b_ptr[nb] + kk));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u32x4 v = zero;
      if (a_ok[mt]) v = *reinterpret_cast<const u32x4*>(a_ptr[mt] + kk);
      abuf[p][mt] = v;
    }
  };
  auto mfma_gran = [&](int p) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const bf16x8_vec afrag = as_bf16x8(abuf[p][mt]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[mt][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag, as_bf16x8(bbuf[p][nb]), acc[mt][nb], 0, 0, 0);
    }
  };

#pragma unroll
  for (int p = 0; p < G; ++p)
    if (p < n_g) load_gran(p, p);
  int g = 0;
  for (; g + G < n_g; g += G) {
#pragma unroll
    for (int p = 0; p < G; ++p) {
      mfma_gran(p);
      if (g + p + G < n_g) load_gran(p, g + p + G);
    }
  }
#pragma unroll
  for (int p = 0; p < G; ++p)
    if (g + p < n_g) mfma_gran(p);

  // K-split reduce: waves 1-3 -> LDS, wave 0 adds them in wave order
  if (wave > 0) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        red[wave - 1][mt * NB + nb][lane] = acc[mt][nb];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const f32x4 o = red[s][mt * NB + nb][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][nb][r] += o[r];
      }

  // C layout: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = tile * R + mt * 16 + koct * 4 + r;
      if (sorted[p] < 0) continue;          // pad row: nothing stored
      if (MODE == MODE_GU) {
#pragma unroll
        for (int ct = 0; ct < HALF; ++ct) {
          const float gv = acc[mt][ct][r];
          const float uv = acc[mt][HALF + ct][r];
          const float s = gv / (1.f + __expf(-gv));
          act_out[int64_t(p) * N + panel * PANEL + ct * 16 + jcol] =
              f32_to_bf16(s * uv);
        }
      } else {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          y_out[int64_t(p) * N + panel * PANEL + nb * 16 + jcol] =
              acc[mt][nb][r];
      }
    }
  }
}

// ---------------------------------------------------------------- combine
__global__ __launch_bounds__(256)
void moe_combine_kernel(const float* __restrict__ y,
                        const int32_t* __restrict__ pos,
                        const float* __restrict__ wts,
                        uint16_t* __restrict__ out, int H, int k) {
  const int t = blockIdx.x;
  for (int h = threadIdx.x * 4; h < H; h += 256 * 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const int p = pos[int64_t(t) * k + j];
      if (p < 0) continue;
      const float wj = wts[int64_t(t) * k + j];
      const float4 v =
          *reinterpret_cast<const float4*>(y + int64_t(p) * H + h);
      acc[0] += wj * v.x;
      acc[1] += wj * v.y;
      acc[2] += wj * v.z;
      acc[3] += wj * v.w;
    }
    ushort4 o;
    o.x = f32_to_bf16(acc[0]);
    o.y = f32_to_bf16(acc[1]);
    o.z = f32_to_bf16(acc[2]);
    o.w = f32_to_bf16(acc[3]);
    *reinterpret_cast<ushort4*>(out + int64_t(t) * H + h) = o;
  }
}

template <int MT, int NB, int G>
void launch_gemms(const uint16_t* x, const uint16_t* w_gate_up,
                  const uint16_t* w_down, const int32_t* sorted,
                  const int32_t* tile_expert, const int32_t* n_live,
                  uint16_t* act, float* y, int max_tiles, int k, int H, int I,
                  hipStream_t stream) {
  hipLaunchKernelGGL((moe_gemm_kernel<MT, NB, MODE_GU, G>),
                     dim3(max_tiles * (I / (NB * 8))), dim3(256), 0, stream,
                     x, w_gate_up, sorted, tile_expert, n_live, act, nullptr,
                     I, H, k);
  hipLaunchKernelGGL((moe_gemm_kernel<MT, NB, MODE_DOWN, G>),
                     dim3(max_tiles * (H / (NB * 16))), dim3(256), 0, stream,
                     act, w_down, sorted, tile_expert, n_live, nullptr, y, H,
                     I, k);
}

}  // namespace

int moe_row_tile(int T, int k, int E) {
  return int64_t(T) * k < int64_t(16) * E ? 16 : 64;
}

int moe_max_tiles(int T, int k, int E, int R) {
  const int64_t P = int64_t(T) * k;
  const int64_t ne = P < E ? P : E;
  return int((P + ne * (R - 1)) / R);
}

void launch_moe_route(const uint16_t* logits, int32_t* ids, float* w, int T,
                      int E, int k, bool renorm, hipStream_t stream) {
  hipLaunchKernelGGL(moe_route_kernel,
                     dim3((T + kRouteWaves - 1) / kRouteWaves),
                     dim3(kRouteWaves * 64), 0, stream, logits, ids, w, T, E,
                     k, renorm ? 1 : 0);
}

void launch_moe_mlp(const uint16_t* x, const int32_t* ids, const float* w,
                    const uint16_t* w_gate_up, const uint16_t* w_down,
                    int32_t* sorted, int32_t* tile_expert, int32_t* pos,
                    int32_t* n_live, uint16_t* act, float* y, uint16_t* out,
                    int T, int k, int E, int H, int I, int R,
                    hipStream_t stream) {
  const int max_tiles = moe_max_tiles(T, k, E, R);
  hipLaunchKernelGGL(moe_align_kernel, dim3(E), dim3(256), 0, stream, ids,
                     T * k, E, R, sorted, tile_expert, pos, n_live);
  if (R == 16)
    launch_gemms<1, 2, 8>(x, w_gate_up, w_down, sorted, tile_expert, n_live,
                          act, y, max_tiles, k, H, I, stream);
  else
    launch_gemms<4, 4, 4>(x, w_gate_up, w_down, sorted, tile_expert, n_live,
                          act, y, max_tiles, k, H, I, stream);
  hipLaunchKernelGGL(moe_combine_kernel, dim3(T), dim3(256), 0, stream, y,
                     pos, w, out, H, k);
}

}  // namespace rlli
