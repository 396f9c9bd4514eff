// Paged-KV block copy for forked sequences (n > 1 choices per request):
// for every layer l and pair p, cache[l, dst[p]] = cache[l, src[p]], for
// K and V in ONE launch.  The cache is raw bytes here (bf16, fp8 or f32
// alike): a (layer, block) chunk is H*bs*D*elt contiguous bytes, moved
// as 16-byte vectors with consecutive lanes on consecutive vectors.
//
// Grid: x strides the chunk's vectors, y = 2*layer + (0: K, 1: V),
// z = pair — no divide anywhere, and the (layer, block) offsets are
// 64-bit (a production cache is far beyond 4 GiB per tensor).  A fork
// moves 2*L*chunk bytes per child (~2 MiB for Llama-3-8B), so this is
// plain vector code: two loads in flight per lane and enough workgroups
// (one per 512 vectors of a chunk) to cover the chip, nothing more.
//
// Contract (the caller's): dst ids are unique and disjoint from src ids;
// src may repeat.  Block ids are not validated on the device.

#include "common.h"

#include <algorithm>

namespace rlli {

namespace {

constexpr int ILP = 2;
constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS)
void kv_copy_blocks_kernel(uint4* __restrict__ k_cache,
                           uint4* __restrict__ v_cache,
                           const int32_t* __restrict__ src,
                           const int32_t* __restrict__ dst,
                           int64_t num_blocks, int64_t chunk_vecs) {
  uint4* cache = (blockIdx.y & 1) ? v_cache : k_cache;
  const int64_t layer = blockIdx.y >> 1;
  const int64_t layer_base = layer * num_blocks;
  const uint4* s = cache + (layer_base + int64_t(src[blockIdx.z])) * chunk_vecs;
  uint4* d = cache + (layer_base + int64_t(dst[blockIdx.z])) * chunk_vecs;
  const int64_t stride = int64_t(gridDim.x) * THREADS;
  int64_t v = int64_t(blockIdx.x) * THREADS + threadIdx.x;
  // two loads in flight per lane before the first store (named
  // registers: a small array here was promoted to LDS by the compiler)
  for (; v + stride < chunk_vecs; v += ILP * stride) {
    const uint4 a = s[v];
    const uint4 b = s[v + stride];
    d[v] = a;
    d[v + stride] = b;
  }
  for (; v < chunk_vecs; v += stride) d[v] = s[v];
}

}  // namespace

void launch_kv_copy_blocks(void* k_cache, void* v_cache, const int32_t* src,
                           const int32_t* dst, int n_pairs, int n_layers,
                           int64_t num_blocks, int64_t chunk_bytes,
                           hipStream_t stream) {
  if (n_pairs == 0 || n_layers == 0 || chunk_bytes == 0) return;
  const int64_t chunk_vecs = chunk_bytes / 16;
  const int64_t per_block = int64_t(THREADS) * ILP;
  const int gx = int(std::min<int64_t>((chunk_vecs + per_block - 1) / per_block,
                                       64));
  hipLaunchKernelGGL(kv_copy_blocks_kernel, dim3(gx, 2 * n_layers, n_pairs),
                     dim3(THREADS), 0, stream,
                     reinterpret_cast<uint4*>(k_cache),
                     reinterpret_cast<uint4*>(v_cache), src, dst, num_blocks,
                     chunk_vecs);
}

}  // namespace rlli
