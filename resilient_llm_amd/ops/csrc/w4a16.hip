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
// Zero-point variants (AWQ checkpoints; ZP = true, w4a16_zp.hip):
//   w4a16_zp_linear: ... sum_{k in g} f32(x[m,k]) * (u[n,k] - z[n,g])
//   w4_zp_dequant:   w[n,k] = bf16( f32(s[n,g]) * (u[n,k] - z[n,g]) )
// Same packed nibbles u; scale and zero-point come as one dword
// meta[N, G]: the fp16 scale in the low half, the bf16 of -(128 + z)
// (0xC300 | z, exact) in the high half.  The fifth MFMA then runs against
// the constant 1.0 and accumulates r = sum_k x[m,k]; the group epilogue is
//     acc += s[n,g] * fma(-(128 + z[n,g]), r, pacc)
// - one FMA more per accumulator register per 128 k than the symmetric
// form, still no per-weight work.  awq_repack (w4a16_zp.hip) turns AutoAWQ
// tensors into packed / meta on the device.
//
// Row m of the result depends on row m of x only and is bit-identical for
// every M: the K-slicing and the order of MFMAs into an accumulator
// depend on (N, K) alone; the ring depth only moves loads.  No atomics:
// split-K slices write f32 slabs that a second kernel sums in slice
// order.

#include "w4a16_common.h"

namespace rlli {

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
  launch_w4a16_any<false>(x, packed, s, ws, out, M, N, K, splitk,
                          grp_per_slice, stream);
}

void launch_w4_dequant(const uint32_t* packed, const uint16_t* s,
                       uint16_t* out, int N, int K, hipStream_t stream) {
  launch_w4_dequant_any<false>(packed, s, out, N, K, stream);
}

}  // namespace rlli
