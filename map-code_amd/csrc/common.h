// Shared helpers for the mapx gfx950 kernels: status codes, launch checks, the dynamic-LDS opt-in, Philox RNG and the
// dropout draw, lane-group reductions, float4 helpers, bf16 I/O.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mapx_hip.h"

#define MAPX_OK 0
#define MAPX_EINVAL (-1)
#define MAPX_EHIP (-2)
#define MAPX_EWORKSPACE (-3)

namespace mapx {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return MAPX_EHIP;
  }
  return MAPX_OK;
}

#define MAPX_REQUIRE(cond, ...)          \
  do {                                   \
    if (!(cond)) {                       \
      ::mapx::set_error(__VA_ARGS__);    \
      return MAPX_EINVAL;                \
    }                                    \
  } while (0)

#define MAPX_HIP(call)                                                   \
  do {                                                                   \
    hipError_t e_ = (call);                                              \
    if (e_ != hipSuccess) {                                              \
      ::mapx::set_error("%s: %s", #call, hipGetErrorString(e_));         \
      return MAPX_EHIP;                                                  \
    }                                                                    \
  } while (0)

// Lets `kernels` ask for up to `bytes` of dynamic LDS (the default limit is 64 KB, the CU has 160 KB); the first
// error.  A call site keeps the result in a function-local static, so the attribute is set once.
template <class... K>
inline hipError_t allow_dynamic_lds(size_t bytes, K*... kernels) {
  for (const void* fn : {reinterpret_cast<const void*>(kernels)...}) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

constexpr int kWave = 64;

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Memory-bound kernels: cap the grid at 256 CUs x 8 blocks and grid-stride the rest.
inline int grid_for(int64_t work_items, int block, int max_blocks = 2048) {
  int64_t g = ceil_div(work_items, block);
  if (g < 1) g = 1;
  if (g > max_blocks) g = max_blocks;
  return (int)g;
}

// ---------------------------------------------------------------- Philox4x32-10
// Counter-based RNG: (seed, offset, element index) -> 4 x u32, no state in memory, so a
// kernel replay (hipGraph) with a bumped offset word gives a fresh, reproducible stream.
struct Philox4 {
  uint32_t x, y, z, w;
};

__device__ inline Philox4 philox4x32_10(uint64_t seed, uint64_t ctr_lo, uint64_t ctr_hi) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32);
  uint32_t c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

// u32 -> uniform integer in [0, n) by multiply-shift (bias < n / 2^32).
__device__ inline uint32_t bounded(uint32_t r, uint32_t n) {
  return (uint32_t)(((uint64_t)r * (uint64_t)n) >> 32);
}
// u32 -> uniform float in [0, 1) with 24 random bits.
__device__ inline float unit_float(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

// THE dropout draw: an inverted-dropout mask is never stored, every user regenerates it from
// Philox(seed, counter, drop_offset(offset, offset_dev)), one draw per four consecutive elements of its own counter
// layout (dropout_kernel: flat i / 4; attn.hip, mha.hip: row * ceil(width / 4) + c).  Element e of the draw is kept
// iff its word >= p * 2^32, so P(keep) = 1 - p.
__device__ inline uint32_t drop_threshold(float p) { return (uint32_t)fminf(p * 4294967296.0f, 4294967295.0f); }

// The device word is what a replayed hipGraph bumps between steps.
__device__ inline uint64_t drop_offset(uint64_t offset, const int32_t* offset_dev) {
  return offset + (offset_dev ? (uint64_t)(uint32_t)*offset_dev : 0ull);
}

// Bit e set = element e of the draw is kept.
__device__ inline uint32_t keep_bits4(const Philox4& r, uint32_t thr) {
  return (uint32_t)(r.x >= thr) | ((uint32_t)(r.y >= thr) << 1) | ((uint32_t)(r.z >= thr) << 2) |
         ((uint32_t)(r.w >= thr) << 3);
}

// Wave64 butterfly sum / max over `width` lanes (width a power of two <= 64).
template <int WIDTH, class V = float>
__device__ inline V group_sum(V v) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
template <int WIDTH>
__device__ inline float group_max(float v) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// acc += s * v and s + a . b, one fmaf per term in x, y, z, w order.
__device__ inline void fma4(float4& acc, float s, const float4& v) {
  acc.x = fmaf(s, v.x, acc.x);
  acc.y = fmaf(s, v.y, acc.y);
  acc.z = fmaf(s, v.z, acc.z);
  acc.w = fmaf(s, v.w, acc.w);
}
__device__ inline float dot4(const float4& a, const float4& b, float s) {
  s = fmaf(a.x, b.x, s);
  s = fmaf(a.y, b.y, s);
  s = fmaf(a.z, b.z, s);
  return fmaf(a.w, b.w, s);
}
// (fignn.hip keeps gn_dot4, hand-written v_fmac_f32, for dot products that run side by side: see its comment.)

// THE fp32 sigmoid of a logit (trainer.py:190, torch.sigmoid on fp32): what the evaluation metrics rank and sum
// (metrics.hip) is what a scoring run writes out (score.hip), bit for bit.
__device__ inline float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

// THE log-loss row term on that probability: the clipped probability of the row's own class, in fp64 with sklearn's
// clip to [eps, 1 - eps], eps = 2^-52 (log_loss on a float64 array); the term is -log of it.  What metrics.hip sums
// per row, bootstrap.hip sums with weights.
__device__ inline double logloss_clipped(double p, bool y) {
  const double eps = 2.220446049250313e-16;
  const double q = y ? p : 1.0 - p;
  return q < eps ? eps : (q > 1.0 - eps ? 1.0 - eps : q);
}
__device__ inline double logloss_term(float p32, bool y) { return -log(logloss_clipped((double)p32, y)); }

// ---------------------------------------------------------------- bf16 I/O (bf16 compute mode)
// Kernels templated on an element type T = float | bf16_t differ only here: a load widens to fp32 (exact), all
// arithmetic is fp32, a store rounds to nearest even once (v_cvt_pk_bf16_f32).
typedef __bf16 bf16_t;
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// The C ABI's mapx_bf16 (a uint16_t) as the device element type.
inline const bf16_t* hc(const mapx_bf16* p) { return reinterpret_cast<const bf16_t*>(p); }
inline bf16_t* hm(mapx_bf16* p) { return reinterpret_cast<bf16_t*>(p); }

// Four consecutive elements (16-byte aligned floats / 8-byte aligned bf16) as fp32, and back.
__device__ inline float4 load4(const float* __restrict__ p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline float4 load4(const bf16_t* __restrict__ p) {
  const bf16x4_t v = *reinterpret_cast<const bf16x4_t*>(p);
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ inline void store4(float* __restrict__ p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ inline void store4(bf16_t* __restrict__ p, const float4& v) {
  bf16x4_t o;
  o[0] = (bf16_t)v.x; o[1] = (bf16_t)v.y; o[2] = (bf16_t)v.z; o[3] = (bf16_t)v.w;
  *reinterpret_cast<bf16x4_t*>(p) = o;
}
// Eight fp32 values as one 16-byte bf16 chunk (what a kernel with 8 columns per lane stores).
__device__ inline bf16x8_t bf16x8_of(const float4& a, const float4& b) {
  bf16x8_t o;
  o[0] = (bf16_t)a.x; o[1] = (bf16_t)a.y; o[2] = (bf16_t)a.z; o[3] = (bf16_t)a.w;
  o[4] = (bf16_t)b.x; o[5] = (bf16_t)b.y; o[6] = (bf16_t)b.z; o[7] = (bf16_t)b.w;
  return o;
}

}  // namespace mapx
