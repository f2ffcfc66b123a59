// The split-K combine of the GEMM families (gemm_x3.hip, gemm_bf16.hip): out[i] = sum_s slabs[s][i], added in slab
// order from 0 (deterministic; both forms give the same bits, so which one runs is a matter of alignment only).
#pragma once
#include "common.h"

namespace mapx {

static __global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ slabs, int64_t slab_stride,
                                                                   int nsplit, int64_t n, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < nsplit; ++s) v += slabs[s * slab_stride + i];
    out[i] = v;
  }
}
// 16-byte form (n % 4 == 0, aligned slabs and output): a quarter of the memory instructions; same order of adds
static __global__ void __launch_bounds__(256) splitk_reduce_v4_kernel(const float* __restrict__ slabs,
                                                                      int64_t slab_stride, int nsplit, int64_t n4,
                                                                      float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = reinterpret_cast<const float4*>(slabs)[i];
    v.x += 0.f; v.y += 0.f; v.z += 0.f; v.w += 0.f;          // (0 + x first, as the scalar form adds)
    for (int s = 1; s < nsplit; ++s) {
      const float4 x = reinterpret_cast<const float4*>(slabs + s * slab_stride)[i];
      v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
    }
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

// C [n] = the sum of `nsplit` slabs of the workspace, slab_stride floats apart
static inline void splitk_reduce_launch(const void* ws, int64_t slab_stride, int nsplit, int64_t n, float* C,
                                        hipStream_t stream) {
  if (n % 4 == 0 && slab_stride % 4 == 0 && (uintptr_t)ws % 16 == 0 && (uintptr_t)C % 16 == 0)
    hipLaunchKernelGGL(splitk_reduce_v4_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, stream,
                       static_cast<const float*>(ws), slab_stride, nsplit, n / 4, C);
  else
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream,
                       static_cast<const float*>(ws), slab_stride, nsplit, n, C);
}

}  // namespace mapx
