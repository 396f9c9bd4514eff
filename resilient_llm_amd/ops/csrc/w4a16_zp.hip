// Zero-point W4A16 (AWQ checkpoints): the ZP = true instances of the
// w4a16_common.h kernels (see w4a16.hip for the design) and the device
// repack from AutoAWQ tensors.  A file of its own so that it is compiled
// without the packed fp32 instructions while w4a16.hip compiles as before.

#include "w4a16_common.h"

namespace rlli {

namespace {

// AutoAWQ "GEMM" tensors -> packed / meta.  qweight is K-major with 8
// columns per dword (nibble i = column 8c + {0,2,4,6,1,3,5,7}[i]); packed
// wants 8 k of one column per dword: a transpose through LDS.
// One workgroup per (64-column panel, group), blockIdx.x = panel +
// panels * g so neighbouring workgroups read neighbouring 32-byte runs of
// the same 128 rows.  Thread t loads the 16 bytes (t & 1) of row t >> 1
// of the 128 x 8-dword tile and stores them at row pitch 9: an output
// dword gathers 8 rows of one LDS column, and a wave (one 16-column tile:
// lane = o * 16 + c) then reads, per (j, i), the rows j*32 + o*8 + i at
// dword 2*tile + c/8 - with pitch 8 the four o would share one bank, with
// pitch 9 the 8 distinct addresses fall in 8 banks (72 o mod 32 = 0, 8,
// 16, 24; + 0..7 from the column dword) and the other lanes broadcast.
// Each thread writes its lane's 16 bytes of the (tile, group) run, so a
// wave writes the whole 1 KiB run; threads 0..63 also write the panel's
// meta column for this group.
constexpr int RP_PITCH = 9;

__global__ __launch_bounds__(256)
void awq_repack_kernel(const uint32_t* __restrict__ qweight,  // [K, N/8]
                       const uint32_t* __restrict__ qzeros,   // [G, N/8]
                       const uint16_t* __restrict__ scales,   // [G, N] fp16
                       uint32_t* __restrict__ packed,
                       uint32_t* __restrict__ meta,           // [N_total, G]
                       int N, int K, int col_offset) {
  __shared__ uint32_t tile_lds[GROUP * RP_PITCH];
  const int G = K / GROUP;
  const int n_panels = N / BN;
  const int panel = blockIdx.x % n_panels;
  const int g = blockIdx.x / n_panels;
  const int t = threadIdx.x;
  const int ndw = N / 8;                     // dwords per qweight row

  {
    const int row = t >> 1, half = t & 1;
    const uint4 v = *reinterpret_cast<const uint4*>(
        qweight + (int64_t(g) * GROUP + row) * ndw + panel * 8 + half * 4);
    uint32_t* dst = tile_lds + row * RP_PITCH + half * 4;
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
  }
  __syncthreads();

  const int ct = t >> 6, lane = t & 63;
  const int c = lane & 15, o = lane >> 4;
  // column ct*16 + c of the panel: dword 2*ct + c/8, nibble of column c%8
  const int cd = 2 * ct + (c >> 3);
  const int sh = 4 * (((c & 7) >> 1) | ((c & 1) << 2));
  u32x4 d;
#pragma unroll
  for (int j = 0; j < GRAN; ++j) {
    unsigned acc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned w = tile_lds[(j * 32 + o * 8 + i) * RP_PITCH + cd];
      acc |= ((w >> sh) & 15u) << (4 * (i / 2) + 16 * (i % 2));
    }
    d[j] = acc;
  }
  const int64_t tile = (col_offset + panel * BN) / 16 + ct;
  *reinterpret_cast<u32x4*>(packed + ((tile * G + g) * 64 + lane) * 4) = d;

  if (t < BN) {
    const int n = panel * BN + t;
    const int zsh = 4 * (((t & 7) >> 1) | ((t & 1) << 2));
    const unsigned z = (qzeros[int64_t(g) * ndw + (n >> 3)] >> zsh) & 15u;
    const unsigned sbits = scales[int64_t(g) * N + n];
    meta[int64_t(col_offset + n) * G + g] = ((0xC300u | z) << 16) | sbits;
  }
}

}  // namespace

void launch_w4a16_zp(const uint16_t* x, const uint32_t* packed,
                     const uint32_t* meta, float* ws, uint16_t* out, int M,
                     int N, int K, int splitk, int grp_per_slice,
                     hipStream_t stream) {
  launch_w4a16_any<true>(x, packed, meta, ws, out, M, N, K, splitk,
                         grp_per_slice, stream);
}

void launch_w4_zp_dequant(const uint32_t* packed, const uint32_t* meta,
                          uint16_t* out, int N, int K, hipStream_t stream) {
  launch_w4_dequant_any<true>(packed, meta, out, N, K, stream);
}

void launch_awq_repack(const uint32_t* qweight, const uint32_t* qzeros,
                       const uint16_t* scales, uint32_t* packed,
                       uint32_t* meta, int N, int K, int col_offset,
                       hipStream_t stream) {
  const int blocks = (N / BN) * (K / GROUP);
  hipLaunchKernelGGL(awq_repack_kernel, dim3(blocks), dim3(256), 0, stream,
                     qweight, qzeros, scales, packed, meta, N, K, col_offset);
}

}  // namespace rlli
