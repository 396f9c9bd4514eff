// Per-head q/k RMSNorm + rotary embedding + paged-KV-cache append (Qwen3).
//
// rope_kv.hip with a norm between the projection and the rotation: every
// q head and every k head x[0..D) becomes
//     n = f32(x) * rsqrt(mean(x^2) + eps) * f32(w)
// (rmsnorm.hip's formula, w = q_norm_w or k_norm_w, [D], shared by all
// heads) and n is rotated as rope_kv.hip rotates its input.  n stays in
// f32 registers: the one bf16 rounding is that of the rotated value, so
// the result is within 2^-8 (|n1 c| + |n2 s|) of the exact one, which a
// second rounding between norm and rotation would double.  q and k are
// written back in place, k and v go to the cache slot at cache precision,
// v is not normalised.
//
// rope_kv.hip's split cannot do this: there a thread takes 8 (lo, hi)
// pairs of a head and never sees a head-wide sum.  Here:
//   - one workgroup per token, sized to the token's heads (up to 256
//     threads);
//   - a lane-group of GW = D/8 lanes owns one head, a lane holds 8
//     contiguous dims from one 16-byte load, so every element is loaded
//     once;
//   - mean(x^2) is reduced inside the lane-group on the VALU pipe
//     (group_sum_dpp<GW>);
//   - the rotation partner's NORMALISED value sits GW/2 lanes away and
//     comes by shuffle, as in the fused decode kernel;
//   - a wave covers 64/GW heads per pass; q, k and v heads are dealt to
//     the lane-groups from one loop (a head's kind is group-uniform, so
//     no reduction or shuffle diverges inside a lane-group).
// No LDS.  Layouts (cos_sin, cache, slot_mapping == -1) as in rope_kv.hip.

#include "common.h"

#include <type_traits>

namespace rlli {

namespace {

template <int GW, typename KC>
__global__ __launch_bounds__(256)
void qk_norm_rope_kv_kernel(uint16_t* __restrict__ q,
                            uint16_t* __restrict__ k,
                            const uint16_t* __restrict__ v,
                            const uint16_t* __restrict__ q_norm_w,
                            const uint16_t* __restrict__ k_norm_w,
                            float eps,
                            const int32_t* __restrict__ positions,
                            const float* __restrict__ cos_sin,
                            typename KC::elem* __restrict__ k_cache,
                            typename KC::elem* __restrict__ v_cache,
                            const int32_t* __restrict__ slot_mapping,
                            int n_q_heads, int n_kv_heads, int block_size,
                            int q_stride, int kv_stride) {
  constexpr int D = GW * 8;
  constexpr int HALF = D / 2;
  const int t = blockIdx.x;
  const int group = threadIdx.x / GW;          // lane-group within the WG
  const int n_groups = blockDim.x / GW;
  const int d0 = (threadIdx.x % GW) * 8;
  const bool first_half = d0 < HALF;

  const int32_t slot = slot_mapping[t];
  // per-head cache offset: ((block*n_kv + h)*block_size + row)*D
  const int64_t cache_base =
      slot >= 0 ? (int64_t(slot / block_size) * n_kv_heads * block_size +
                   int64_t(slot % block_size)) * D + d0
                : 0;

  // rope coefficients of this lane's 8 dims (pair index = d mod D/2): the
  // same for every head the lane visits
  const float* cs = cos_sin + int64_t(positions[t]) * D + d0 % HALF;
  const float4 c01 = *reinterpret_cast<const float4*>(cs);
  const float4 c23 = *reinterpret_cast<const float4*>(cs + 4);
  const float4 s01 = *reinterpret_cast<const float4*>(cs + HALF);
  const float4 s23 = *reinterpret_cast<const float4*>(cs + HALF + 4);
  const float cv[8] = {c01.x, c01.y, c01.z, c01.w, c23.x, c23.y, c23.z, c23.w};
  const float sv[8] = {s01.x, s01.y, s01.z, s01.w, s23.x, s23.y, s23.z, s23.w};

  const int n_qk = n_q_heads + n_kv_heads;
  // slot < 0: v has nowhere to go, its heads are not visited
  const int n_heads = slot >= 0 ? n_qk + n_kv_heads : n_qk;
  for (int hh = group; hh < n_heads; hh += n_groups) {
    if (hh >= n_qk) {
      // ---- v head: copy into the cache at cache precision ----
      const int h = hh - n_qk;
      bf16x8 vv;
      vv.u = *reinterpret_cast<const uint4*>(
          v + int64_t(t) * kv_stride + h * D + d0);
      float vf[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) vf[i] = bf16_to_f32(vv.s[i]);
      *reinterpret_cast<typename KC::vec8*>(
          v_cache + cache_base + int64_t(h) * block_size * D) =
          KC::from_f32(vf);
      continue;
    }
    const bool is_q = hh < n_q_heads;
    const int h = is_q ? hh : hh - n_q_heads;
    uint16_t* base = is_q ? q + int64_t(t) * q_stride + h * D + d0
                          : k + int64_t(t) * kv_stride + h * D + d0;
    bf16x8 xv, wv;
    xv.u = *reinterpret_cast<const uint4*>(base);
    wv.u = *reinterpret_cast<const uint4*>((is_q ? q_norm_w : k_norm_w) + d0);

    // ---- RMSNorm over the head, kept in f32 ----
    float x[8], ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      x[i] = bf16_to_f32(xv.s[i]);
      ss += x[i] * x[i];
    }
    ss = group_sum_dpp<GW>(ss);
    const float inv = rsqrtf(ss / D + eps);
    float n[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      n[i] = x[i] * inv * bf16_to_f32(wv.s[i]);

    // ---- rotate: the partner of dim d is d +- D/2, GW/2 lanes away ----
    float r[8];
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float other = __shfl_xor(n[i], GW / 2, kWave);
      r[i] = first_half ? n[i] * cv[i] - other * sv[i]
                        : n[i] * cv[i] + other * sv[i];
      o.s[i] = f32_to_bf16(r[i]);
    }
    *reinterpret_cast<uint4*>(base) = o.u;
    if (!is_q && slot >= 0)
      *reinterpret_cast<typename KC::vec8*>(
          k_cache + cache_base + int64_t(h) * block_size * D) =
          KC::from_f32(r);
  }
}

template <int GW, typename KC>
void launch(uint16_t* q, uint16_t* k, const uint16_t* v,
            const uint16_t* q_norm_w, const uint16_t* k_norm_w, float eps,
            const int32_t* positions, const float* cos_sin, void* k_cache,
            void* v_cache, const int32_t* slot_mapping, int tokens,
            int n_q_heads, int n_kv_heads, int block_size, int q_stride,
            int kv_stride, hipStream_t stream) {
  // whole waves covering every head once, at most 256 threads (then a
  // lane-group takes several heads)
  const int lanes = (n_q_heads + 2 * n_kv_heads) * GW;
  const int threads = lanes >= 256 ? 256 : (lanes + kWave - 1) / kWave * kWave;
  hipLaunchKernelGGL((qk_norm_rope_kv_kernel<GW, KC>), dim3(tokens),
                     dim3(threads), 0, stream, q, k, v, q_norm_w, k_norm_w,
                     eps, positions, cos_sin,
                     static_cast<typename KC::elem*>(k_cache),
                     static_cast<typename KC::elem*>(v_cache), slot_mapping,
                     n_q_heads, n_kv_heads, block_size, q_stride, kv_stride);
}

}  // namespace

void launch_qk_norm_rope_kv_append(
    uint16_t* q, uint16_t* k, uint16_t* v,
    const uint16_t* q_norm_w, const uint16_t* k_norm_w, float eps,
    const int32_t* positions, const float* cos_sin,
    void* k_cache, void* v_cache,
    const int32_t* slot_mapping,
    int tokens, int n_q_heads, int n_kv_heads, int head_dim,
    int block_size, int q_stride, int kv_stride, bool cache_fp8,
    hipStream_t stream) {
  if (tokens == 0) return;
  auto run = [&](auto gw_tag) {
    constexpr int GW = decltype(gw_tag)::value;
    if (cache_fp8)
      launch<GW, CacheFP8>(q, k, v, q_norm_w, k_norm_w, eps, positions,
                           cos_sin, k_cache, v_cache, slot_mapping, tokens,
                           n_q_heads, n_kv_heads, block_size, q_stride,
                           kv_stride, stream);
    else
      launch<GW, CacheBF16>(q, k, v, q_norm_w, k_norm_w, eps, positions,
                            cos_sin, k_cache, v_cache, slot_mapping, tokens,
                            n_q_heads, n_kv_heads, block_size, q_stride,
                            kv_stride, stream);
  };
  if (head_dim == 128) run(std::integral_constant<int, 16>{});
  else if (head_dim == 64) run(std::integral_constant<int, 8>{});
  // other head dims: the caller validates
}

}  // namespace rlli
