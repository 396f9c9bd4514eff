// SwiGLU fused into the W4A16 decode down projection: the SILU = true
// instances of the w4a16_common.h kernel (see w4a16.hip for the format and
// the design), symmetric and zero-point.
//
//   out[m,n] = bf16( sum_g s[n,g] * sum_{k in g} a[m,k] * q[n,k] )
//   a[m,k]   = bf16( silu(f32(gu[m,k])) * f32(gu[m,K+k]) ),   1 <= M <= 64
//
// gu [M, 2K] is what the gate_up projection writes.  A wave loads the gate
// and the up octet of every row tile into the granule slot the plain
// kernel keeps one octet in, and turns them into the A fragment with
// silu_mul_bf16 (common.h, the expression silu_mul.hip stores) right
// before the slot's MFMAs: 8 values per lane per row tile per granule, in
// every one of the N / 64 panels.  The weight ring, the K-slicing
// (w4a16_plan), the order of MFMAs into an accumulator, the group epilogue,
// the f32 slab and its reduce are the plain kernel's, so the result is
// bit-identical to w4a16_linear(silu_mul(gu)), for every M, with one
// launch and the [M, K] intermediate less.
//
// A file of its own so that it is compiled without the packed fp32
// instructions while w4a16.hip compiles as before.

#include "w4a16_common.h"

namespace rlli {

void launch_w4a16_silu(const uint16_t* gu, const uint32_t* packed,
                       const uint16_t* s, float* ws, uint16_t* out, int M,
                       int N, int K, int splitk, int grp_per_slice,
                       hipStream_t stream) {
  launch_w4a16_any<false, true>(gu, packed, s, ws, out, M, N, K, splitk,
                                grp_per_slice, stream);
}

void launch_w4a16_zp_silu(const uint16_t* gu, const uint32_t* packed,
                          const uint32_t* meta, float* ws, uint16_t* out,
                          int M, int N, int K, int splitk, int grp_per_slice,
                          hipStream_t stream) {
  launch_w4a16_any<true, true>(gu, packed, meta, ws, out, M, N, K, splitk,
                               grp_per_slice, stream);
}

}  // namespace rlli
