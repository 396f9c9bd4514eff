// Torch bindings for the gfx950 kernels (TORCH_LIBRARY, not pybind — the
// ops dispatch through torch.ops.rlli.* and stay graph-capturable).
// This is the only translation unit that includes torch headers; the
// kernels live in pure-HIP .hip files behind kernels.h.

#include <torch/library.h>
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>

#include "kernels.h"

#include <cstdlib>
#include <vector>

namespace {

using at::Tensor;

hipStream_t current_stream(const Tensor& t) {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA(
      t.device().index()).stream();
}

// after-launch error check (skipped inside hipGraph capture, where the
// runtime reports capture-sequencing pseudo-errors)
void check_launch(const char* op) {
  if (c10::hip::currentStreamCaptureStatusMayInitCtx() !=
      c10::hip::CaptureStatus::None)
    return;
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, op, " launch failed: ", hipGetErrorString(e));
}

uint16_t* bf16_ptr(const Tensor& t) {
  return reinterpret_cast<uint16_t*>(t.data_ptr());
}

void check_bf16_contig(const Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
}


// cache tensors: bf16 or fp8-e4m3 (common.h codecs); returns the fp8
// flag after validating dtype/contiguity/device
bool check_cache(const Tensor& k_cache, const Tensor& v_cache) {
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(),
              "k/v cache dtype mismatch");
  const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || k_cache.scalar_type() == at::kBFloat16,
              "kv cache must be bf16 or float8_e4m3fn");
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous() &&
              k_cache.is_cuda() && v_cache.is_cuda());
  return fp8;
}

// ------------------------------------------------------------- rmsnorm
Tensor rmsnorm(const Tensor& x, const Tensor& w, double eps) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w, "w");
  const int dim = int(x.size(-1));
  TORCH_CHECK(dim % 8 == 0, "dim must be a multiple of 8");
  TORCH_CHECK(w.numel() == dim, "weight/dim mismatch");
  const int rows = int(x.numel() / dim);
  Tensor y = at::empty_like(x);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_rmsnorm(bf16_ptr(x), nullptr, bf16_ptr(w), bf16_ptr(y), rows,
                       dim, float(eps), current_stream(x));
  check_launch("rmsnorm");
  return y;
}

Tensor rmsnorm_residual_(const Tensor& x, Tensor residual, const Tensor& w,
                         double eps) {
  check_bf16_contig(x, "x");
  check_bf16_contig(residual, "residual");
  check_bf16_contig(w, "w");
  TORCH_CHECK(x.sizes() == residual.sizes(), "x/residual shape mismatch");
  const int dim = int(x.size(-1));
  TORCH_CHECK(dim % 8 == 0 && w.numel() == dim, "bad dim/weight");
  const int rows = int(x.numel() / dim);
  Tensor y = at::empty_like(x);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_rmsnorm(bf16_ptr(x), bf16_ptr(residual), bf16_ptr(w),
                       bf16_ptr(y), rows, dim, float(eps), current_stream(x));
  check_launch("rmsnorm_residual_");
  return y;
}

// ---- fp8-activation emitters (quantized-weight GEMM path) ----
std::tuple<Tensor, Tensor> rmsnorm_fp8(const Tensor& x, const Tensor& w,
                                       double eps) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w, "w");
  const int dim = int(x.size(-1));
  TORCH_CHECK(dim % 8 == 0 && dim <= 8192 && w.numel() == dim,
              "bad dim/weight for fp8 rmsnorm");
  const int rows = int(x.numel() / dim);
  Tensor y8 = at::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
  Tensor scales = at::empty({rows}, x.options().dtype(at::kFloat));
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_rmsnorm_fp8(bf16_ptr(x), nullptr, bf16_ptr(w),
                           reinterpret_cast<uint8_t*>(y8.data_ptr()),
                           scales.data_ptr<float>(), rows, dim, float(eps),
                           current_stream(x));
  check_launch("rmsnorm_fp8");
  return {y8, scales};
}

std::tuple<Tensor, Tensor> rmsnorm_residual_fp8(const Tensor& x,
                                                Tensor residual,
                                                const Tensor& w, double eps) {
  check_bf16_contig(x, "x");
  check_bf16_contig(residual, "residual");
  check_bf16_contig(w, "w");
  TORCH_CHECK(x.sizes() == residual.sizes(), "x/residual shape mismatch");
  const int dim = int(x.size(-1));
  TORCH_CHECK(dim % 8 == 0 && dim <= 8192 && w.numel() == dim,
              "bad dim/weight for fp8 rmsnorm");
  const int rows = int(x.numel() / dim);
  Tensor y8 = at::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
  Tensor scales = at::empty({rows}, x.options().dtype(at::kFloat));
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_rmsnorm_fp8(bf16_ptr(x), bf16_ptr(residual), bf16_ptr(w),
                           reinterpret_cast<uint8_t*>(y8.data_ptr()),
                           scales.data_ptr<float>(), rows, dim, float(eps),
                           current_stream(x));
  check_launch("rmsnorm_residual_fp8");
  return {y8, scales};
}

std::tuple<Tensor, Tensor> silu_mul_fp8(const Tensor& gate_up) {
  check_bf16_contig(gate_up, "gate_up");
  const int64_t inter = gate_up.size(-1) / 2;
  TORCH_CHECK(inter % 8 == 0, "inter must be a multiple of 8");
  const int rows = int(gate_up.numel() / (2 * inter));
  auto sizes = gate_up.sizes().vec();
  sizes.back() = inter;
  Tensor y8 = at::empty(sizes, gate_up.options().dtype(at::kFloat8_e4m3fn));
  Tensor scales = at::empty({rows}, gate_up.options().dtype(at::kFloat));
  c10::hip::HIPGuardMasqueradingAsCUDA guard(gate_up.device());
  rlli::launch_silu_mul_fp8(bf16_ptr(gate_up),
                            reinterpret_cast<uint8_t*>(y8.data_ptr()),
                            scales.data_ptr<float>(), rows, int(inter),
                            current_stream(gate_up));
  check_launch("silu_mul_fp8");
  return {y8, scales};
}

// ------------------------------------------------------------ silu_mul
Tensor silu_mul(const Tensor& gate_up) {
  check_bf16_contig(gate_up, "gate_up");
  const int twoi = int(gate_up.size(-1));
  TORCH_CHECK(twoi % 16 == 0, "2*intermediate must be a multiple of 16");
  const int inter = twoi / 2;
  const int rows = int(gate_up.numel() / twoi);
  auto sizes = gate_up.sizes().vec();
  sizes.back() = inter;
  Tensor y = at::empty(sizes, gate_up.options());
  c10::hip::HIPGuardMasqueradingAsCUDA guard(gate_up.device());
  rlli::launch_silu_mul(bf16_ptr(gate_up), bf16_ptr(y), rows, inter,
                        current_stream(gate_up));
  check_launch("silu_mul");
  return y;
}

// ------------------------------------------------------- rope_kv_append
void rope_kv_append_(Tensor q, Tensor k, const Tensor& v,
                     const Tensor& positions, const Tensor& cos_sin,
                     Tensor k_cache, Tensor v_cache,
                     const Tensor& slot_mapping) {
  check_bf16_contig(q, "q");
  check_bf16_contig(k, "k");
  check_bf16_contig(v, "v");
  const bool cache_fp8 = check_cache(k_cache, v_cache);
  TORCH_CHECK(positions.scalar_type() == at::kInt && positions.is_contiguous());
  TORCH_CHECK(slot_mapping.scalar_type() == at::kInt && slot_mapping.is_contiguous());
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous());
  const int tokens = int(q.size(0));
  const int n_q = int(q.size(1));
  const int n_kv = int(k.size(1));
  const int D = int(q.size(2));
  TORCH_CHECK(k.size(2) == D && v.size(1) == n_kv && v.size(2) == D);
  TORCH_CHECK(D % 16 == 0, "head_dim must be a multiple of 16");
  TORCH_CHECK(cos_sin.size(1) == D, "cos_sin must be [max_pos, head_dim]");
  TORCH_CHECK(k_cache.size(1) == n_kv && k_cache.size(3) == D);
  const int block_size = int(k_cache.size(2));
  TORCH_CHECK(positions.numel() == tokens && slot_mapping.numel() == tokens);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(q.device());
  rlli::launch_rope_kv_append(
      bf16_ptr(q), bf16_ptr(k), bf16_ptr(v),
      positions.data_ptr<int32_t>(), cos_sin.data_ptr<float>(),
      k_cache.data_ptr(), v_cache.data_ptr(),
      slot_mapping.data_ptr<int32_t>(),
      tokens, n_q, n_kv, D, block_size, n_q * D, n_kv * D, cache_fp8,
      current_stream(q));
  check_launch("rope_kv_append_");
}

// Fused-QKV form: qkv is the raw [T, (n_q + 2*n_kv) * D] GEMM output;
// rope + cache append run on strided views, zero copies.
void rope_kv_append_qkv_(Tensor qkv, const Tensor& positions,
                         const Tensor& cos_sin, Tensor k_cache,
                         Tensor v_cache, const Tensor& slot_mapping,
                         int64_t n_q) {
  check_bf16_contig(qkv, "qkv");
  const bool cache_fp8 = check_cache(k_cache, v_cache);
  const int n_kv = int(k_cache.size(1));
  const int D = int(k_cache.size(3));
  const int block_size = int(k_cache.size(2));
  const int stride = int(qkv.size(1));
  TORCH_CHECK(stride == (n_q + 2 * n_kv) * D, "qkv width mismatch");
  const int tokens = int(qkv.size(0));
  TORCH_CHECK(positions.numel() == tokens && slot_mapping.numel() == tokens);
  TORCH_CHECK(cos_sin.size(1) == D && D % 16 == 0);
  uint16_t* base = bf16_ptr(qkv);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  rlli::launch_rope_kv_append(
      base, base + n_q * D, base + (n_q + n_kv) * D,
      positions.data_ptr<int32_t>(), cos_sin.data_ptr<float>(),
      k_cache.data_ptr(), v_cache.data_ptr(),
      slot_mapping.data_ptr<int32_t>(),
      tokens, int(n_q), n_kv, D, block_size, stride, stride, cache_fp8,
      current_stream(qkv));
  check_launch("rope_kv_append_qkv_");
}


// split-K scratch for decode attention (empty tensors when n_split==1);
// allocation participates in hipGraph capture pools, so graphed decode
// buckets capture their scratch once and reuse it on replay.
struct SplitScratch {
  int n_split = 1;
  Tensor part, ml;
  float* part_ptr() { return n_split > 1 ? part.data_ptr<float>() : nullptr; }
  float* ml_ptr() { return n_split > 1 ? ml.data_ptr<float>() : nullptr; }
};

static SplitScratch make_split_scratch(const Tensor& ref, int batch,
                                       int n_kv, int group, int D) {
  SplitScratch s;
  static const bool disabled = std::getenv("RLLI_NO_SPLITK") != nullptr;
  if (disabled) return s;
  s.n_split = rlli::decode_attn_n_split(batch, n_kv);
  if (s.n_split > 1) {
    auto opt = ref.options().dtype(at::kFloat);
    s.part = at::empty({int64_t(batch) * n_kv * s.n_split * group * D}, opt);
    s.ml = at::empty({int64_t(batch) * n_kv * s.n_split * group * 2}, opt);
  }
  return s;
}

// Introspection for tests: the split factor decode_attn /
// decode_attn_qkv / decode_attn_rope_qkv run with at this (batch, n_kv).
// It asks make_split_scratch itself (group = D = 1: a few host floats),
// so it cannot drift from what the ops do.
int64_t decode_attn_split(int64_t batch, int64_t n_kv) {
  TORCH_CHECK(batch >= 1 && n_kv >= 1 && batch * n_kv < (int64_t(1) << 24),
              "bad batch/n_kv");
  const Tensor host = at::empty({0}, at::TensorOptions().dtype(at::kFloat));
  return make_split_scratch(host, int(batch), int(n_kv), 1, 1).n_split;
}

// ---------------------------------------------------------- decode_attn
Tensor decode_attn(const Tensor& q, const Tensor& k_cache,
                   const Tensor& v_cache, const Tensor& block_table,
                   const Tensor& seq_lens, double scale) {
  check_bf16_contig(q, "q");
  const bool cache_fp8 = check_cache(k_cache, v_cache);
  TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.is_contiguous());
  TORCH_CHECK(seq_lens.scalar_type() == at::kInt && seq_lens.is_contiguous());
  const int batch = int(q.size(0));
  const int n_q = int(q.size(1));
  const int D = int(q.size(2));
  const int n_kv = int(k_cache.size(1));
  const int block_size = int(k_cache.size(2));
  const int max_blocks = int(block_table.size(1));
  const int group = n_q / n_kv;
  TORCH_CHECK(n_q % n_kv == 0 && (group == 1 || group == 2 || group == 4 || group == 8),
              "GQA group must be 1/2/4/8, got ", group);
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128, got ", D);
  const int gpw = 64 / (D / 8);
  TORCH_CHECK(block_size % gpw == 0, "block_size must be a multiple of ", gpw);
  TORCH_CHECK(k_cache.size(3) == D && v_cache.sizes() == k_cache.sizes());
  TORCH_CHECK(block_table.size(0) == batch && seq_lens.numel() == batch);
  Tensor out = at::empty_like(q);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(q.device());
  SplitScratch ss = make_split_scratch(q, batch, n_kv, group, D);
  rlli::launch_decode_attn(
      bf16_ptr(q), k_cache.data_ptr(), v_cache.data_ptr(),
      block_table.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
      bf16_ptr(out), batch, n_q, n_kv, D, block_size, max_blocks,
      float(scale), n_q * D, ss.n_split, ss.part_ptr(), ss.ml_ptr(),
      cache_fp8, current_stream(q));
  check_launch("decode_attn");
  return out;
}

// Fused-QKV decode attention: q read strided from the qkv GEMM output.
Tensor decode_attn_qkv(const Tensor& qkv, const Tensor& k_cache,
                       const Tensor& v_cache, const Tensor& block_table,
                       const Tensor& seq_lens, double scale, int64_t n_q) {
  check_bf16_contig(qkv, "qkv");
  const bool cache_fp8 = check_cache(k_cache, v_cache);
  const int batch = int(qkv.size(0));
  const int n_kv = int(k_cache.size(1));
  const int D = int(k_cache.size(3));
  const int block_size = int(k_cache.size(2));
  const int max_blocks = int(block_table.size(1));
  const int stride = int(qkv.size(1));
  TORCH_CHECK(stride == (n_q + 2 * n_kv) * D, "qkv width mismatch");
  const int group = int(n_q) / n_kv;
  TORCH_CHECK(group == 1 || group == 2 || group == 4 || group == 8);
  TORCH_CHECK(D == 64 || D == 128);
  Tensor out = at::empty({batch, n_q * D}, qkv.options());
  c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  SplitScratch ss = make_split_scratch(qkv, batch, n_kv, group, D);
  rlli::launch_decode_attn(
      bf16_ptr(qkv), k_cache.data_ptr(), v_cache.data_ptr(),
      block_table.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
      bf16_ptr(out), batch, int(n_q), n_kv, D, block_size, max_blocks,
      float(scale), stride, ss.n_split, ss.part_ptr(), ss.ml_ptr(),
      cache_fp8, current_stream(qkv));
  check_launch("decode_attn_qkv");
  return out;
}

// Fused decode: rope + append + attention in one kernel.
Tensor decode_attn_rope_qkv(const Tensor& qkv, const Tensor& positions,
                            const Tensor& cos_sin, Tensor k_cache,
                            Tensor v_cache, const Tensor& slot_mapping,
                            const Tensor& block_table, const Tensor& seq_lens,
                            double scale, int64_t n_q) {
  check_bf16_contig(qkv, "qkv");
  const bool cache_fp8 = check_cache(k_cache, v_cache);
  TORCH_CHECK(positions.scalar_type() == at::kInt && positions.is_contiguous());
  TORCH_CHECK(slot_mapping.scalar_type() == at::kInt && slot_mapping.is_contiguous());
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous());
  TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.is_contiguous());
  TORCH_CHECK(seq_lens.scalar_type() == at::kInt && seq_lens.is_contiguous());
  const int batch = int(qkv.size(0));
  const int n_kv = int(k_cache.size(1));
  const int block_size = int(k_cache.size(2));
  const int D = int(k_cache.size(3));
  const int stride = int(qkv.size(1));
  TORCH_CHECK(stride == (n_q + 2 * n_kv) * D, "qkv width mismatch");
  const int group = int(n_q) / n_kv;
  TORCH_CHECK(group == 1 || group == 2 || group == 4 || group == 8);
  TORCH_CHECK(D == 64 || D == 128);
  TORCH_CHECK(cos_sin.size(1) == D);
  const int max_blocks = int(block_table.size(1));
  Tensor out = at::empty({batch, n_q * D}, qkv.options());
  c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  SplitScratch ss = make_split_scratch(qkv, batch, n_kv, group, D);
  rlli::launch_decode_attn_fused(
      bf16_ptr(qkv), k_cache.data_ptr(), v_cache.data_ptr(),
      block_table.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
      positions.data_ptr<int32_t>(), cos_sin.data_ptr<float>(),
      slot_mapping.data_ptr<int32_t>(), bf16_ptr(out), batch, int(n_q),
      n_kv, D, block_size, max_blocks, float(scale), stride,
      ss.n_split, ss.part_ptr(), ss.ml_ptr(), cache_fp8,
      current_stream(qkv));
  check_launch("decode_attn_rope_qkv");
  return out;
}

// --------------------------------------------------------- prefill_attn
Tensor prefill_attn(const Tensor& q, const Tensor& k, const Tensor& v,
                    const Tensor& cu_seqlens, double scale) {
  check_bf16_contig(q, "q");
  check_bf16_contig(k, "k");
  check_bf16_contig(v, "v");
  TORCH_CHECK(cu_seqlens.scalar_type() == at::kInt && cu_seqlens.is_contiguous());
  const int T = int(q.size(0));
  const int n_q = int(q.size(1));
  const int D = int(q.size(2));
  const int n_kv = int(k.size(1));
  const int group = n_q / n_kv;
  TORCH_CHECK(n_q % n_kv == 0 && (group == 1 || group == 2 || group == 4 || group == 8),
              "GQA group must be 1/2/4/8, got ", group);
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(k.size(0) == T && v.size(0) == T && k.size(2) == D);
  const int n_seqs = int(cu_seqlens.numel()) - 1;
  Tensor out = at::empty_like(q);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(q.device());
  rlli::launch_prefill_attn(
      bf16_ptr(q), bf16_ptr(k), bf16_ptr(v), cu_seqlens.data_ptr<int32_t>(),
      bf16_ptr(out), n_seqs, T, n_q, n_kv, D, float(scale),
      n_q * D, n_kv * D, current_stream(q));
  check_launch("prefill_attn");
  return out;
}

// Fused-QKV prefill attention: q/k/v all read strided from qkv (k was
// rope-rotated in place by rope_kv_append_qkv_).
Tensor prefill_attn_qkv(const Tensor& qkv, const Tensor& cu_seqlens,
                        double scale, int64_t n_q, int64_t n_kv,
                        int64_t head_dim) {
  check_bf16_contig(qkv, "qkv");
  TORCH_CHECK(cu_seqlens.scalar_type() == at::kInt && cu_seqlens.is_contiguous());
  const int T = int(qkv.size(0));
  const int D = int(head_dim);
  const int stride = int(qkv.size(1));
  TORCH_CHECK(stride == (n_q + 2 * n_kv) * D, "qkv width mismatch");
  const int group = int(n_q) / int(n_kv);
  TORCH_CHECK(group == 1 || group == 2 || group == 4 || group == 8);
  TORCH_CHECK(D == 64 || D == 128);
  const int n_seqs = int(cu_seqlens.numel()) - 1;
  Tensor out = at::empty({T, n_q * D}, qkv.options());
  c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  // chunk tables for the MFMA kernel (host-side; prefill is not captured)
  Tensor cu_cpu = cu_seqlens.to(at::kCPU);
  const int32_t* cu = cu_cpu.data_ptr<int32_t>();
  std::vector<int32_t> t0s, starts, ends;
  for (int s = 0; s < n_seqs; ++s)
    for (int t = cu[s]; t < cu[s + 1]; t += 32) {
      t0s.push_back(t);
      starts.push_back(cu[s]);
      ends.push_back(cu[s + 1]);
    }
  const int n_chunks = int(t0s.size());
  auto iopt = at::TensorOptions().dtype(at::kInt);
  Tensor t0_d = at::tensor(t0s, iopt).to(qkv.device(), /*nb=*/true);
  Tensor st_d = at::tensor(starts, iopt).to(qkv.device(), true);
  Tensor en_d = at::tensor(ends, iopt).to(qkv.device(), true);
  rlli::launch_prefill_mfma(
      bf16_ptr(qkv), t0_d.data_ptr<int32_t>(), st_d.data_ptr<int32_t>(),
      en_d.data_ptr<int32_t>(), bf16_ptr(out), n_chunks, int(n_kv),
      group, D, stride, float(scale), current_stream(qkv));
  check_launch("prefill_attn_qkv");
  return out;
}

// ------------------------------------------------------ prefill (paged)
Tensor prefill_paged_attn(const Tensor& qkv, const Tensor& k_cache,
                          const Tensor& v_cache, const Tensor& chunk_row0,
                          const Tensor& chunk_pos0, const Tensor& chunk_nrows,
                          const Tensor& chunk_btrow,
                          const Tensor& block_tables, double scale,
                          int64_t n_q) {
  check_bf16_contig(qkv, "qkv");
  const bool cache_fp8 = check_cache(k_cache, v_cache);
  for (const Tensor* t : {&chunk_row0, &chunk_pos0, &chunk_nrows,
                          &chunk_btrow, &block_tables}) {
    TORCH_CHECK(t->scalar_type() == at::kInt && t->is_contiguous() &&
                t->is_cuda(), "chunk/table tensors must be contiguous "
                "int32 on the GPU");
  }
  const int T = int(qkv.size(0));
  const int n_kv = int(k_cache.size(1));
  const int block_size = int(k_cache.size(2));
  const int D = int(k_cache.size(3));
  const int stride = int(qkv.size(1));
  TORCH_CHECK(stride >= n_q * D, "qkv too narrow");
  const int group = int(n_q) / n_kv;
  TORCH_CHECK(group == 1 || group == 2 || group == 4 || group == 8);
  TORCH_CHECK(D == 64 || D == 128);
  const int n_chunks = int(chunk_row0.numel());
  const int max_blocks = int(block_tables.size(1));
  Tensor out = at::empty({T, n_q * D}, qkv.options());
  c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  rlli::launch_prefill_paged(
      bf16_ptr(qkv), k_cache.data_ptr(), v_cache.data_ptr(),
      chunk_row0.data_ptr<int32_t>(), chunk_pos0.data_ptr<int32_t>(),
      chunk_nrows.data_ptr<int32_t>(), chunk_btrow.data_ptr<int32_t>(),
      block_tables.data_ptr<int32_t>(), bf16_ptr(out), n_chunks, n_kv,
      group, D, stride, max_blocks, block_size, float(scale), cache_fp8,
      current_stream(qkv));
  check_launch("prefill_paged_attn");
  return out;
}

// --------------------------------------------------------- skinny_linear
Tensor skinny_linear(const Tensor& x, const Tensor& w) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w, "w");
  const int M = int(x.size(0));
  const int K = int(x.size(1));
  const int N = int(w.size(0));
  TORCH_CHECK(w.size(1) == K, "x/W K mismatch");
  TORCH_CHECK(M >= 1 && M <= 64, "skinny_linear needs 1 <= M <= 64, got ", M);
  TORCH_CHECK(K % 256 == 0 && N % 64 == 0,
              "skinny_linear needs K%256==0 and N%64==0, got K=", K, " N=", N);
  const int n_panels = N / 64;
  int splitk = 1;
  if (n_panels < 256) {
    splitk = std::min<int>(8, std::max<int>(1, 512 / n_panels));
    splitk = std::min<int>(splitk, K / 256);
  }
  Tensor out = at::empty({M, N}, x.options());
  Tensor ws;
  float* ws_ptr = nullptr;
  if (splitk > 1) {
    ws = at::empty({splitk, M, N}, x.options().dtype(at::kFloat));
    ws_ptr = ws.data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_skinny_gemm(bf16_ptr(x), bf16_ptr(w), ws_ptr, bf16_ptr(out),
                           M, N, K, splitk, current_stream(x));
  check_launch("skinny_linear");
  return out;
}

// ------------------------------------------------------------- skinny2
// v2 zero-LDS skinny GEMM; splitk <= 0 picks the grid-fill heuristic
// (>= ~512 workgroups).  Requirements: M <= 64, K % 256 == 0, N % 16 == 0.
static int skinny2_auto_splitk(int N, int K) {
  const int panels = N / 64;   // one 64-column panel per wave
  int sk = std::max(1, (512 + panels - 1) / panels);
  return std::min<int>(sk, std::max(1, K / 256));
}

Tensor skinny2_linear(const Tensor& x, const Tensor& w, int64_t splitk) {
  check_bf16_contig(x, "x");
  check_bf16_contig(w, "w");
  const int M = int(x.size(0));
  const int K = int(x.size(1));
  const int N = int(w.size(0));
  TORCH_CHECK(w.size(1) == K, "x/W K mismatch");
  TORCH_CHECK(M >= 1 && M <= 64, "skinny2_linear needs 1 <= M <= 64, got ", M);
  TORCH_CHECK(K % 256 == 0 && N % 64 == 0,
              "skinny2_linear needs K%256==0 and N%64==0, got K=", K, " N=", N);
  int sk = int(splitk) > 0 ? int(splitk) : skinny2_auto_splitk(N, K);
  sk = std::min(sk, K / 256);
  Tensor out = at::empty({M, N}, x.options());
  Tensor ws;
  float* ws_ptr = nullptr;
  if (sk > 1) {
    ws = at::empty({sk, M, N}, x.options().dtype(at::kFloat));
    ws_ptr = ws.data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_skinny2(bf16_ptr(x), bf16_ptr(w), ws_ptr, bf16_ptr(out),
                       M, N, K, sk, current_stream(x));
  check_launch("skinny2_linear");
  return out;
}

// down-proj with the SwiGLU fused into the A-fragment path:
// out = (silu(gu[:, :K]) * gu[:, K:]) @ w^T,  gu = [M, 2K].
Tensor skinny2_silu_linear(const Tensor& gu, const Tensor& w, int64_t splitk) {
  check_bf16_contig(gu, "gu");
  check_bf16_contig(w, "w");
  const int M = int(gu.size(0));
  const int K2 = int(gu.size(1));
  TORCH_CHECK(K2 % 2 == 0, "gu must be [M, 2K]");
  const int K = K2 / 2;
  const int N = int(w.size(0));
  TORCH_CHECK(w.size(1) == K, "gu/W K mismatch");
  TORCH_CHECK(M >= 1 && M <= 64, "skinny2_silu needs 1 <= M <= 64, got ", M);
  TORCH_CHECK(K % 256 == 0 && N % 64 == 0,
              "skinny2_silu needs K%256==0 and N%64==0, got K=", K, " N=", N);
  int sk = int(splitk) > 0 ? int(splitk) : skinny2_auto_splitk(N, K);
  sk = std::min(sk, K / 256);
  Tensor out = at::empty({M, N}, gu.options());
  Tensor ws;
  float* ws_ptr = nullptr;
  if (sk > 1) {
    ws = at::empty({sk, M, N}, gu.options().dtype(at::kFloat));
    ws_ptr = ws.data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(gu.device());
  rlli::launch_skinny2_silu(bf16_ptr(gu), bf16_ptr(w), ws_ptr, bf16_ptr(out),
                            M, N, K, sk, current_stream(gu));
  check_launch("skinny2_silu_linear");
  return out;
}

// --------------------------------------------------------------- w4a16
// int4 group-quantized weights: packed int32 [N*K/8] in the fragment
// order of ops/ref.py w4_pack, s bf16 [N, K/128].
void check_w4(const Tensor& packed, const Tensor& s, const Tensor& like) {
  TORCH_CHECK(s.dim() == 2 && s.size(0) >= 1 && s.size(1) >= 1,
              "s must be [N, K/128]");
  check_bf16_contig(s, "s");
  const int64_t N = s.size(0), K = s.size(1) * 128;
  TORCH_CHECK(N % 64 == 0, "int4 weights need N % 64 == 0, got N=", N);
  TORCH_CHECK(N * K / 2 < (int64_t(1) << 31), "int4 weight too large");
  TORCH_CHECK(packed.scalar_type() == at::kInt && packed.is_contiguous() &&
              packed.is_cuda(), "packed must be contiguous int32 on the GPU");
  TORCH_CHECK(packed.numel() == N * K / 8, "packed must hold N*K/8 = ",
              N * K / 8, " elements, got ", packed.numel());
  TORCH_CHECK(packed.device() == like.device() &&
              s.device() == like.device(), "device mismatch");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed.data_ptr()) % 16 == 0,
              "packed must be 16-byte aligned");
}

// the K-slicing w4a16_linear runs with: [slices, k per slice]
std::vector<int64_t> w4a16_plan(int64_t N, int64_t K, int64_t splitk) {
  TORCH_CHECK(N >= 64 && N % 64 == 0 && K >= 128 && K % 128 == 0 &&
              N < (int64_t(1) << 24) && K < (int64_t(1) << 24),
              "w4a16 needs N % 64 == 0 and K % 128 == 0");
  int sk = 1, gps = 1;
  rlli::w4a16_plan(int(N), int(K), int(splitk), &sk, &gps);
  return {sk, int64_t(gps) * 128};
}

// out [M, N] bf16 is written in full and nothing else is, apart from the
// first slices*M*N floats of the split-K slab: ``ws`` when the caller
// owns one (>= that many f32), else a caching-allocator tensor, which
// inside hipGraph capture comes from the graph's pool.
void w4a16_linear_(const Tensor& x, const Tensor& packed, const Tensor& s,
                   int64_t splitk, Tensor out,
                   const c10::optional<Tensor>& ws_opt) {
  check_bf16_contig(x, "x");
  check_bf16_contig(out, "out");
  TORCH_CHECK(x.dim() == 2, "x must be [M, K]");
  check_w4(packed, s, x);
  const int M = int(x.size(0));
  const int K = int(x.size(1));
  const int N = int(s.size(0));
  TORCH_CHECK(M >= 1 && M <= 64, "w4a16_linear needs 1 <= M <= 64, got ", M);
  TORCH_CHECK(K % 128 == 0 && K >= 128,
              "w4a16_linear needs K % 128 == 0, got K=", K);
  TORCH_CHECK(s.size(1) * 128 == K, "x/s K mismatch: x has K=", K,
              ", s has ", s.size(1), " groups");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "x must be 16-byte aligned");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == N &&
              out.device() == x.device(), "out must be [M, N] = [", M, ", ",
              N, "] on x's device");
  int sk = 1, gps = 1;
  rlli::w4a16_plan(N, K, int(splitk), &sk, &gps);
  Tensor ws;
  float* ws_ptr = nullptr;
  if (sk > 1) {
    if (ws_opt.has_value()) {
      ws = *ws_opt;
      TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.is_contiguous() &&
                  ws.device() == x.device() &&
                  ws.numel() >= int64_t(sk) * M * N,
                  "ws must be contiguous f32 with >= slices*M*N = ",
                  int64_t(sk) * M * N, " elements on x's device");
    } else {
      ws = at::empty({sk, M, N}, x.options().dtype(at::kFloat));
    }
    ws_ptr = ws.data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_w4a16(bf16_ptr(x),
                     reinterpret_cast<const uint32_t*>(packed.data_ptr()),
                     bf16_ptr(s), ws_ptr, bf16_ptr(out), M, N, K, sk, gps,
                     current_stream(x));
  check_launch("w4a16_linear");
}

void w4_dequant_(const Tensor& packed, const Tensor& s, Tensor out) {
  check_bf16_contig(out, "out");
  check_w4(packed, s, out);
  const int64_t N = s.size(0), K = s.size(1) * 128;
  TORCH_CHECK(out.dim() == 2 && out.size(0) == N && out.size(1) == K,
              "out must be [N, K] = [", N, ", ", K, "]");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(out.device());
  rlli::launch_w4_dequant(
      reinterpret_cast<const uint32_t*>(packed.data_ptr()), bf16_ptr(s),
      bf16_ptr(out), int(N), int(K), current_stream(out));
  check_launch("w4_dequant_");
}

Tensor stream_probe(const Tensor& w, int64_t splitk) {
  check_bf16_contig(w, "w");
  Tensor sink = at::zeros({256}, w.options().dtype(at::kFloat));
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  rlli::launch_stream_probe(bf16_ptr(w), sink.data_ptr<float>(),
                            int(w.size(0)), int(w.size(1)), int(splitk),
                            current_stream(w));
  check_launch("stream_probe");
  return sink;
}

// --------------------------------------------------------------- sample
Tensor sample(const Tensor& logits, const Tensor& temperatures,
              const Tensor& seeds, int64_t step) {
  check_bf16_contig(logits, "logits");
  TORCH_CHECK(temperatures.scalar_type() == at::kFloat &&
              temperatures.is_contiguous() && temperatures.is_cuda());
  TORCH_CHECK(seeds.scalar_type() == at::kLong && seeds.is_contiguous() &&
              seeds.is_cuda());
  const int batch = int(logits.size(0));
  const int vocab = int(logits.size(1));
  TORCH_CHECK(temperatures.numel() == batch && seeds.numel() == batch);
  Tensor out = at::empty({batch}, logits.options().dtype(at::kInt));
  c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  const int n_split = rlli::sample_n_split(batch);
  uint64_t* pptr = nullptr;
  Tensor partials;
  if (n_split > 1) {
    // caching-allocator tensor: participates in hipGraph capture pools
    partials = at::empty({int64_t(batch) * n_split},
                         logits.options().dtype(at::kLong));
    pptr = reinterpret_cast<uint64_t*>(partials.data_ptr<int64_t>());
  }
  rlli::launch_sample(bf16_ptr(logits), temperatures.data_ptr<float>(),
                      reinterpret_cast<const uint64_t*>(seeds.data_ptr<int64_t>()),
                      uint64_t(step), out.data_ptr<int32_t>(), batch, vocab,
                      pptr, n_split, current_stream(logits));
  check_launch("sample");
  return out;
}

// --------------------------------------------------- sample_constrained
// rows / bias_offsets / bias_ids VALUES are trusted (as slot_mapping is);
// the kernel still clamps the CSR slice and ignores ids outside the vocab.
Tensor sample_constrained(const Tensor& logits, const Tensor& rows,
                          const Tensor& temperatures, const Tensor& seeds,
                          int64_t step, const Tensor& top_k,
                          const Tensor& min_p, const Tensor& bias_offsets,
                          const Tensor& bias_ids, const Tensor& bias_vals) {
  check_bf16_contig(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) >= 1,
              "logits must be [B, V] with V >= 1");
  for (const Tensor* t : {&rows, &top_k, &bias_offsets, &bias_ids}) {
    TORCH_CHECK(t->scalar_type() == at::kInt && t->is_contiguous() &&
                t->is_cuda() && t->device() == logits.device(),
                "rows/top_k/bias_offsets/bias_ids must be contiguous int32 "
                "on the logits' device");
  }
  for (const Tensor* t : {&temperatures, &min_p, &bias_vals}) {
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() &&
                t->is_cuda() && t->device() == logits.device(),
                "temperatures/min_p/bias_vals must be contiguous float32 "
                "on the logits' device");
  }
  TORCH_CHECK(seeds.scalar_type() == at::kLong && seeds.is_contiguous() &&
              seeds.is_cuda() && seeds.device() == logits.device(),
              "seeds must be contiguous int64 on the logits' device");
  const int64_t batch = logits.size(0);
  const int64_t vocab = logits.size(1);
  TORCH_CHECK(temperatures.numel() == batch && seeds.numel() == batch,
              "temperatures/seeds must have one entry per logits row");
  const int64_t n_rows = rows.numel();
  TORCH_CHECK(top_k.numel() == n_rows && min_p.numel() == n_rows &&
              bias_offsets.numel() == n_rows + 1,
              "rows/top_k/min_p/bias_offsets length mismatch");
  TORCH_CHECK(bias_ids.numel() == bias_vals.numel(),
              "bias_ids/bias_vals length mismatch");
  TORCH_CHECK(bias_ids.numel() < (int64_t(1) << 31), "bias list too long");
  TORCH_CHECK(vocab <= rlli::sample_constrained_max_vocab(),
              "sample_constrained supports vocab <= ",
              rlli::sample_constrained_max_vocab(), ", got ", vocab);
  Tensor out = at::empty({n_rows}, logits.options().dtype(at::kInt));
  if (n_rows == 0) return out;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  rlli::launch_sample_constrained(
      bf16_ptr(logits), rows.data_ptr<int32_t>(),
      temperatures.data_ptr<float>(),
      reinterpret_cast<const uint64_t*>(seeds.data_ptr<int64_t>()),
      uint64_t(step), top_k.data_ptr<int32_t>(), min_p.data_ptr<float>(),
      bias_offsets.data_ptr<int32_t>(), bias_ids.data_ptr<int32_t>(),
      bias_vals.data_ptr<float>(), int(bias_ids.numel()),
      out.data_ptr<int32_t>(), int(n_rows), int(vocab),
      current_stream(logits));
  check_launch("sample_constrained");
  return out;
}

// ------------------------------------------------------- token_logprobs
// rows/tokens VALUES are trusted (as slot_mapping is): rows index
// logits' first dim, tokens its second.
std::tuple<Tensor, Tensor, Tensor> token_logprobs(const Tensor& logits,
                                                  const Tensor& rows,
                                                  const Tensor& tokens,
                                                  int64_t k) {
  check_bf16_contig(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) >= 1,
              "logits must be [B, V] with V >= 1");
  for (const Tensor* t : {&rows, &tokens}) {
    TORCH_CHECK(t->scalar_type() == at::kInt && t->is_contiguous() &&
                t->is_cuda() && t->device() == logits.device(),
                "rows/tokens must be contiguous int32 on the logits' device");
  }
  TORCH_CHECK(tokens.numel() == rows.numel(), "rows/tokens length mismatch");
  const int64_t vocab = logits.size(1);
  TORCH_CHECK(vocab < (int64_t(1) << 30), "vocab too large");
  TORCH_CHECK(k >= 0 && k <= 20 && k <= vocab,
              "k must be in [0, min(20, vocab)], got ", k);
  const int n_rows = int(rows.numel());
  auto fopt = logits.options().dtype(at::kFloat);
  Tensor chosen_lp = at::empty({n_rows}, fopt);
  Tensor top_lp = at::empty({n_rows, k}, fopt);
  Tensor top_ids = at::empty({n_rows, k}, logits.options().dtype(at::kInt));
  if (n_rows == 0) return {chosen_lp, top_lp, top_ids};
  c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  const int n_split = rlli::logprobs_n_split(n_rows, int(vocab));
  Tensor stats = at::empty({n_rows, n_split, 2}, fopt);
  Tensor cand = at::empty({n_rows, n_split, k},
                          logits.options().dtype(at::kLong));
  rlli::launch_token_logprobs(
      bf16_ptr(logits), rows.data_ptr<int32_t>(), tokens.data_ptr<int32_t>(),
      chosen_lp.data_ptr<float>(), top_lp.data_ptr<float>(),
      top_ids.data_ptr<int32_t>(), n_rows, int(vocab), int(k),
      stats.data_ptr<float>(),
      reinterpret_cast<uint64_t*>(cand.data_ptr<int64_t>()), n_split,
      current_stream(logits));
  check_launch("token_logprobs");
  return {chosen_lp, top_lp, top_ids};
}

// ------------------------------------------------------- kv_copy_blocks_
// cache[l, dst[p]] = cache[l, src[p]] for every layer, K and V, in one
// launch on raw bytes (any 1/2/4-byte element).  src/dst VALUES are
// trusted (as slot_mapping is): dst unique and disjoint from src.
void kv_copy_blocks_(Tensor k_cache, Tensor v_cache, const Tensor& src,
                     const Tensor& dst) {
  TORCH_CHECK(k_cache.dim() == 5 && k_cache.sizes() == v_cache.sizes(),
              "k/v cache must both be [L, NB, H, bs, D]");
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(),
              "k/v cache dtype mismatch");
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous(),
              "k/v cache must be contiguous");
  TORCH_CHECK(k_cache.is_cuda() && v_cache.device() == k_cache.device(),
              "k/v cache must be on the same GPU");
  const int64_t elt = k_cache.element_size();
  TORCH_CHECK(elt == 1 || elt == 2 || elt == 4,
              "kv cache element size must be 1, 2 or 4 bytes, got ", elt);
  for (const Tensor* t : {&src, &dst}) {
    TORCH_CHECK(t->scalar_type() == at::kInt && t->is_contiguous() &&
                t->dim() == 1 && t->device() == k_cache.device(),
                "src/dst must be contiguous 1-D int32 on the cache's device");
  }
  TORCH_CHECK(src.numel() == dst.numel(), "src/dst length mismatch");
  const int64_t n_pairs = src.numel();
  const int64_t n_layers = k_cache.size(0);
  const int64_t chunk_bytes =
      k_cache.size(2) * k_cache.size(3) * k_cache.size(4) * elt;
  TORCH_CHECK(chunk_bytes % 16 == 0,
              "a (layer, block) chunk must be a multiple of 16 bytes, got ",
              chunk_bytes);
  TORCH_CHECK(n_pairs <= 65535 && 2 * n_layers <= 65535,
              "too many pairs/layers for one launch");
  if (n_pairs == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(k_cache.device());
  rlli::launch_kv_copy_blocks(k_cache.data_ptr(), v_cache.data_ptr(),
                              src.data_ptr<int32_t>(),
                              dst.data_ptr<int32_t>(), int(n_pairs),
                              int(n_layers), k_cache.size(1), chunk_bytes,
                              current_stream(k_cache));
  check_launch("kv_copy_blocks_");
}

// ------------------------------------------------------------------ lora
// Batched multi-adapter LoRA (lora.hip).  adapter_idx VALUES are checked
// on the device: a row whose index is negative or past the stack is a
// no-adapter row.
void check_adapter_idx(const Tensor& idx, const Tensor& like, int64_t T) {
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.is_contiguous() &&
              idx.dim() == 1 && idx.numel() == T &&
              idx.device() == like.device(),
              "adapter_idx must be contiguous int32 [T] on the data's device");
}

// y[T, R] f32; rows with adapter_idx -1 are NOT written (unspecified).
Tensor lora_shrink(const Tensor& x, const Tensor& A,
                   const Tensor& adapter_idx) {
  check_bf16_contig(x, "x");
  check_bf16_contig(A, "A");
  TORCH_CHECK(x.dim() == 2 && A.dim() == 3 && A.size(2) == x.size(1),
              "x must be [T, K] and A [n_adapters, R, K]");
  TORCH_CHECK(A.device() == x.device(), "x/A device mismatch");
  const int64_t T = x.size(0), K = x.size(1), R = A.size(1);
  TORCH_CHECK(R >= 1 && R <= 192, "stacked rank R must be in 1..192, got ", R);
  TORCH_CHECK(K >= 1 && T <= INT32_MAX && K <= INT32_MAX);
  check_adapter_idx(adapter_idx, x, T);
  Tensor y = at::empty({T, R}, x.options().dtype(at::kFloat));
  if (T == 0) return y;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  rlli::launch_lora_shrink(bf16_ptr(x), bf16_ptr(A),
                           adapter_idx.data_ptr<int32_t>(),
                           y.data_ptr<float>(), int(T), int(A.size(0)),
                           int(R), int(K), current_stream(x));
  check_launch("lora_shrink");
  return y;
}

void lora_expand_add_(Tensor out, const Tensor& y, const Tensor& B,
                      const Tensor& scale, at::IntArrayRef slices,
                      const Tensor& adapter_idx) {
  check_bf16_contig(out, "out");
  check_bf16_contig(B, "B");
  TORCH_CHECK(out.dim() == 2 && B.dim() == 3 && B.size(1) == out.size(1),
              "out must be [T, O] and B [n_adapters, O, r_max]");
  const int64_t T = out.size(0), O = out.size(1), r_max = B.size(2);
  const int64_t n_slices = int64_t(slices.size());
  TORCH_CHECK(r_max >= 1 && r_max <= 64, "r_max must be in 1..64, got ", r_max);
  TORCH_CHECK(n_slices >= 1 && n_slices <= 3,
              "slices holds 1..3 end-exclusive row boundaries");
  int ends[3] = {0, 0, 0};
  int64_t prev = 0;
  for (int64_t i = 0; i < n_slices; ++i) {
    TORCH_CHECK(slices[i] > prev && slices[i] <= O,
                "slice boundaries must ascend within (0, O]");
    prev = slices[i];
    ends[i] = int(slices[i]);
  }
  TORCH_CHECK(prev == O, "the last slice boundary must equal O");
  TORCH_CHECK(y.scalar_type() == at::kFloat && y.is_contiguous() &&
              y.dim() == 2 && y.size(0) == T &&
              y.size(1) == n_slices * r_max && y.device() == out.device(),
              "y must be contiguous f32 [T, n_slices * r_max]");
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.is_contiguous() &&
              scale.dim() == 1 && scale.numel() == B.size(0) &&
              scale.device() == out.device(),
              "scale must be contiguous f32 [n_adapters]");
  TORCH_CHECK(B.device() == out.device(), "out/B device mismatch");
  TORCH_CHECK(T <= INT32_MAX && O <= INT32_MAX - 256);
  check_adapter_idx(adapter_idx, out, T);
  if (T == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(out.device());
  rlli::launch_lora_expand_add(bf16_ptr(out), y.data_ptr<float>(),
                               bf16_ptr(B), scale.data_ptr<float>(),
                               adapter_idx.data_ptr<int32_t>(), int(T),
                               int(B.size(0)), int(O), int(r_max),
                               int(n_slices), ends, current_stream(out));
  check_launch("lora_expand_add_");
}

}  // namespace

TORCH_LIBRARY(rlli, m) {
  m.def("rmsnorm(Tensor x, Tensor w, float eps) -> Tensor");
  m.def("rmsnorm_residual_(Tensor x, Tensor(a!) residual, Tensor w, float eps) -> Tensor");
  m.def("silu_mul(Tensor gate_up) -> Tensor");
  m.def("rmsnorm_fp8(Tensor x, Tensor w, float eps) -> (Tensor, Tensor)");
  m.def("rmsnorm_residual_fp8(Tensor x, Tensor(a!) residual, Tensor w, float eps) -> (Tensor, Tensor)");
  m.def("silu_mul_fp8(Tensor gate_up) -> (Tensor, Tensor)");
  m.def("rope_kv_append_(Tensor(a!) q, Tensor(b!) k, Tensor v, Tensor positions, "
        "Tensor cos_sin, Tensor(c!) k_cache, Tensor(d!) v_cache, "
        "Tensor slot_mapping) -> ()");
  m.def("decode_attn(Tensor q, Tensor k_cache, Tensor v_cache, "
        "Tensor block_table, Tensor seq_lens, float scale) -> Tensor");
  m.def("decode_attn_split(int batch, int n_kv) -> int", &decode_attn_split);
  m.def("rope_kv_append_qkv_(Tensor(a!) qkv, Tensor positions, Tensor cos_sin, "
        "Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor slot_mapping, "
        "int n_q) -> ()");
  m.def("decode_attn_qkv(Tensor qkv, Tensor k_cache, Tensor v_cache, "
        "Tensor block_table, Tensor seq_lens, float scale, int n_q) -> Tensor");
  m.def("decode_attn_rope_qkv(Tensor qkv, Tensor positions, Tensor cos_sin, "
        "Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor slot_mapping, "
        "Tensor block_table, Tensor seq_lens, float scale, int n_q) -> Tensor");
  m.def("prefill_attn_qkv(Tensor qkv, Tensor cu_seqlens, float scale, "
        "int n_q, int n_kv, int head_dim) -> Tensor");
  m.def("prefill_attn(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens, "
        "float scale) -> Tensor");
  m.def("sample(Tensor logits, Tensor temperatures, Tensor seeds, int step) -> Tensor");
  m.def("sample_constrained(Tensor logits, Tensor rows, Tensor temperatures, "
        "Tensor seeds, int step, Tensor top_k, Tensor min_p, "
        "Tensor bias_offsets, Tensor bias_ids, Tensor bias_vals) -> Tensor");
  m.def("token_logprobs(Tensor logits, Tensor rows, Tensor tokens, int k) "
        "-> (Tensor, Tensor, Tensor)");
  m.def("skinny_linear(Tensor x, Tensor w) -> Tensor");
  m.def("skinny2_linear(Tensor x, Tensor w, int splitk) -> Tensor");
  m.def("skinny2_silu_linear(Tensor gu, Tensor w, int splitk) -> Tensor");
  m.def("w4a16_linear_(Tensor x, Tensor packed, Tensor s, int splitk, "
        "Tensor(a!) out, Tensor(b!)? ws) -> ()");
  m.def("w4a16_plan(int N, int K, int splitk) -> int[]", &w4a16_plan);
  m.def("w4_dequant_(Tensor packed, Tensor s, Tensor(a!) out) -> ()");
  m.def("stream_probe(Tensor w, int splitk) -> Tensor");
  m.def("prefill_paged_attn(Tensor qkv, Tensor k_cache, Tensor v_cache, "
        "Tensor chunk_row0, Tensor chunk_pos0, Tensor chunk_nrows, "
        "Tensor chunk_btrow, Tensor block_tables, float scale, int n_q) "
        "-> Tensor");
  m.def("kv_copy_blocks_(Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor src, "
        "Tensor dst) -> ()");
  m.def("lora_shrink(Tensor x, Tensor A, Tensor adapter_idx) -> Tensor");
  m.def("lora_expand_add_(Tensor(a!) out, Tensor y, Tensor B, Tensor scale, "
        "int[] slices, Tensor adapter_idx) -> ()");
}

TORCH_LIBRARY_IMPL(rlli, CUDA, m) {
  m.impl("rmsnorm", &rmsnorm);
  m.impl("rmsnorm_residual_", &rmsnorm_residual_);
  m.impl("silu_mul", &silu_mul);
  m.impl("rmsnorm_fp8", &rmsnorm_fp8);
  m.impl("rmsnorm_residual_fp8", &rmsnorm_residual_fp8);
  m.impl("silu_mul_fp8", &silu_mul_fp8);
  m.impl("rope_kv_append_", &rope_kv_append_);
  m.impl("decode_attn", &decode_attn);
  m.impl("rope_kv_append_qkv_", &rope_kv_append_qkv_);
  m.impl("decode_attn_qkv", &decode_attn_qkv);
  m.impl("decode_attn_rope_qkv", &decode_attn_rope_qkv);
  m.impl("prefill_attn_qkv", &prefill_attn_qkv);
  m.impl("prefill_attn", &prefill_attn);
  m.impl("sample", &sample);
  m.impl("sample_constrained", &sample_constrained);
  m.impl("token_logprobs", &token_logprobs);
  m.impl("skinny_linear", &skinny_linear);
  m.impl("skinny2_linear", &skinny2_linear);
  m.impl("skinny2_silu_linear", &skinny2_silu_linear);
  m.impl("w4a16_linear_", &w4a16_linear_);
  m.impl("w4_dequant_", &w4_dequant_);
  m.impl("stream_probe", &stream_probe);
  m.impl("prefill_paged_attn", &prefill_paged_attn);
  m.impl("kv_copy_blocks_", &kv_copy_blocks_);
  m.impl("lora_shrink", &lora_shrink);
  m.impl("lora_expand_add_", &lora_expand_add_);
}
