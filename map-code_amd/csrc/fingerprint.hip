// Order-independent 64-bit integer fingerprint of a buffer of 32-bit words (include/mapx_hip.h:
// mapx_fingerprint_words; DESIGN §5 "Replica-consistency check").  All arithmetic is unsigned 64-bit and wraps:
//   mix(x):  x += G;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^ x >> 31
//   chunk k (65536 words, the last one may be short):  c_k = sum_j mix(j << 32 | w[k * 65536 + j])
//   buffer:                                            F   = sum_k mix(c_k + (k + 1) * G)
// Both sums commute, so the result is exact for any grid and any wave order: no atomics, no floating point.  One
// workgroup per chunk (grid-striding), 16-byte loads on the aligned body; the base is only 4-byte aligned (parameters
// are views into flat buffers), so up to 3 head words and up to 3 tail words of a chunk are read one by one.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr int kFpBlock = 256;
constexpr int64_t kFpChunk = 65536;
constexpr uint64_t kFpG = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t fp_mix(uint64_t x) {
  x += kFpG;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ uint64_t fp_word(uint32_t j, uint32_t w) { return fp_mix(((uint64_t)j << 32) | w); }

// Sum over the workgroup's kFpBlock threads; the result is valid in thread 0.  `part` holds one slot per wave and
// may be reused by the next call: the leading barrier orders that call's writes behind this call's reads.
__device__ __forceinline__ uint64_t fp_block_sum(uint64_t v, uint64_t* part) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, kWave);
  __syncthreads();
  if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = v;
  __syncthreads();
  uint64_t s = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kFpBlock / kWave; ++i) s += part[i];
  }
  return s;
}

__global__ void __launch_bounds__(kFpBlock) fingerprint_chunks_kernel(const uint32_t* __restrict__ w, int64_t n,
                                                                      int64_t nchunks, uint64_t* __restrict__ chunks) {
  __shared__ uint64_t part[kFpBlock / kWave];
  const int tid = threadIdx.x;
  for (int64_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint32_t* base = w + k * kFpChunk;
    const int len = (int)min(kFpChunk, n - k * kFpChunk);
    // words in front of the first 16-byte boundary (the same for every chunk: a chunk is 256 KiB)
    const int head = min(len, (int)(((16u - (uint32_t)((uintptr_t)base & 15u)) & 15u) >> 2));
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const uint4* body = reinterpret_cast<const uint4*>(base + head);
    uint64_t acc = 0;
    int v = tid;
    for (; v + 3 * kFpBlock < nvec; v += 4 * kFpBlock) {      // four 16-byte loads in flight per lane
      uint4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = body[v + u * kFpBlock];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t j = (uint32_t)(head + 4 * (v + u * kFpBlock));
        acc += fp_word(j, q[u].x) + fp_word(j + 1, q[u].y) + fp_word(j + 2, q[u].z) + fp_word(j + 3, q[u].w);
      }
    }
    for (; v < nvec; v += kFpBlock) {
      const uint4 q = body[v];
      const uint32_t j = (uint32_t)(head + 4 * v);
      acc += fp_word(j, q.x) + fp_word(j + 1, q.y) + fp_word(j + 2, q.z) + fp_word(j + 3, q.w);
    }
    if (tid < head) acc += fp_word((uint32_t)tid, base[tid]);
    if (tail0 + tid < len) acc += fp_word((uint32_t)(tail0 + tid), base[tail0 + tid]);
    const uint64_t c = fp_block_sum(acc, part);
    if (tid == 0) chunks[k] = c;
  }
}

__global__ void __launch_bounds__(kFpBlock) fingerprint_fold_kernel(const uint64_t* __restrict__ chunks, int64_t nchunks,
                                                                    uint64_t* __restrict__ total) {
  __shared__ uint64_t part[kFpBlock / kWave];
  uint64_t acc = 0;
  for (int64_t k = threadIdx.x; k < nchunks; k += kFpBlock) acc += fp_mix(chunks[k] + (uint64_t)(k + 1) * kFpG);
  const uint64_t f = fp_block_sum(acc, part);
  if (threadIdx.x == 0) *total = f;
}

}  // namespace mapx

extern "C" int mapx_fingerprint_words(const void* data, int64_t n_words, uint64_t* chunks, uint64_t* total, int blocks,
                                      hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(total && n_words >= 0 && blocks >= 0, "fingerprint_words: bad arguments");
  MAPX_REQUIRE(n_words == 0 || (data && chunks), "fingerprint_words: null buffer");
  MAPX_REQUIRE((uintptr_t)data % 4 == 0 && (uintptr_t)chunks % 8 == 0 && (uintptr_t)total % 8 == 0,
               "fingerprint_words: data must be 4-byte, chunks and total 8-byte aligned");
  const int64_t nchunks = ceil_div(n_words, kFpChunk);
  if (nchunks > 0) {
    const int64_t cap = blocks > 0 ? blocks : 2048;      // auto: 256 CUs x 8 workgroups, grid-striding beyond
    const int grid = (int)(nchunks < cap ? nchunks : cap);
    hipLaunchKernelGGL(fingerprint_chunks_kernel, dim3(grid), dim3(kFpBlock), 0, stream,
                       static_cast<const uint32_t*>(data), n_words, nchunks, chunks);
    if (int st = check_launch("fingerprint_chunks")) return st;
  }
  hipLaunchKernelGGL(fingerprint_fold_kernel, dim3(1), dim3(kFpBlock), 0, stream, chunks, nchunks, total);
  return check_launch("fingerprint_fold");
}
