// Options of the hot-path classes that the DCNv2 run scripts leave off but the CLI accepts:
// dropout (reference code/layers.py:95 Embeddings.dropout, :183 MLPBlock's nn.Dropout) and the
// embeddings' LayerNorm (layers.py:92-94, 99-100).  HBM-bound elementwise / row kernels.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

// Inverted dropout, mask never stored: element i keeps its value iff bit i % 4 of the dropout draw (common.h) at
// counter i / 4 is set, scaled by 1 / (1 - p).  Forward and backward call the same kernel with the
// same (seed, offset): the mask is regenerated, not saved (0 bytes of activation memory, graph-replay
// safe through the device-side offset).
// T: float, or bf16_t (bf16 compute mode: x * scale in fp32, rounded once; the mask does not depend on T).  `vec`
// (bf16 only): x and out are 8-byte aligned, so a thread's four elements move as one load and one store.
template <class T>
__global__ void __launch_bounds__(256) dropout_kernel(const T* __restrict__ x, int64_t n, float p, float scale,
                                                      uint64_t seed, uint64_t offset,
                                                      const int32_t* __restrict__ offset_dev,
                                                      T* __restrict__ out, int vec) {
  const uint64_t off = drop_offset(offset, offset_dev);
  const uint32_t thr = drop_threshold(p);
  const int64_t n4 = (n + 3) / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t keep = keep_bits4(philox4x32_10(seed, (uint64_t)i, off), thr);
    if constexpr (sizeof(T) == 2) {
      if (vec && 4 * i + 4 <= n) {
        const float4 v = load4(x + 4 * i);
        store4(out + 4 * i, make_float4((keep & 1u) ? v.x * scale : 0.f, (keep & 2u) ? v.y * scale : 0.f,
                                        (keep & 4u) ? v.z * scale : 0.f, (keep & 8u) ? v.w * scale : 0.f));
        continue;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t j = 4 * i + e;
      if (j < n) out[j] = (T)(((keep >> e) & 1u) ? (float)x[j] * scale : 0.f);
    }
  }
}

// LayerNorm over the last dimension E (<= 64, E % 4 == 0) of [R, E]: one lane group of E/4 lanes per row.
//   y = (v - mean) * rstd * w + b,  rstd = 1 / sqrt(var + eps)  (biased variance, as nn.LayerNorm),  v = x + s
// T = float: the embeddings' LayerNorm (s = null).  T = bf16_t: residual add + LayerNorm of the Transformer's bf16
// trunk (s = null: LN(x)); the sum is formed in fp32 from the two bf16 addends and normalised as it stands — it is
// never stored, so it is never rounded; y is rounded once.
template <int LG, class T>
__global__ void __launch_bounds__(256) layernorm_fwd_kernel(const T* __restrict__ x, const T* __restrict__ s, int64_t R,
                                                            int E, const float* __restrict__ w,
                                                            const float* __restrict__ b, float eps, T* __restrict__ y,
                                                            float* __restrict__ stats /* [R,2] mean, rstd */) {
  const int lig = threadIdx.x % LG;
  const bool live = lig * 4 < E;
  const float4 wv = live ? *reinterpret_cast<const float4*>(w + 4 * lig) : make_float4(0, 0, 0, 0);
  const float4 bv = live ? *reinterpret_cast<const float4*>(b + 4 * lig) : make_float4(0, 0, 0, 0);
  for (int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LG; row < R;
       row += ((int64_t)gridDim.x * blockDim.x) / LG) {
    float4 v = live ? load4(x + row * E + 4 * lig) : make_float4(0, 0, 0, 0);
    if (s && live) {
      const float4 a = load4(s + row * E + 4 * lig);
      v = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
    }
    const float mean = group_sum<LG>(v.x + v.y + v.z + v.w) / E;
    const float4 d = make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
    const float var = group_sum<LG>(live ? d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w : 0.f) / E;
    const float rstd = rsqrtf(var + eps);
    if (live)
      store4(y + row * E + 4 * lig, make_float4(d.x * rstd * wv.x + bv.x, d.y * rstd * wv.y + bv.y,
                                                d.z * rstd * wv.z + bv.z, d.w * rstd * wv.w + bv.w));
    if (lig == 0) {
      stats[2 * row] = mean;
      stats[2 * row + 1] = rstd;
    }
  }
}

// A lane's four columns of one row in backward: v = x + s (s = null: x) and dy in, then
//   xhat = (v - mean) * rstd,  g = dy * w,  dv = rstd * (g - mean(g) - xhat * mean(g * xhat))  stored to dx.
// Every lane of a wave calls it (the group_sum shuffles need all 64); `have` = this lane has a live column of a row
// < R.  Returns dy and xhat, from which the callers form dw and db in their own ways.
template <int LG, class T>
__device__ inline void layernorm_bwd_row(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ s,
                                         const float4& wv, float mean, float rstd, int64_t row, int E, int lig,
                                         bool have, T* __restrict__ dx, float4& gy, float4& xh) {
  float4 v = have ? load4(x + row * E + 4 * lig) : make_float4(0, 0, 0, 0);
  if (s && have) {
    const float4 a = load4(s + row * E + 4 * lig);
    v = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
  }
  gy = have ? load4(dy + row * E + 4 * lig) : make_float4(0, 0, 0, 0);
  xh = make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd);
  const float4 g = make_float4(gy.x * wv.x, gy.y * wv.y, gy.z * wv.z, gy.w * wv.w);
  const float mg = group_sum<LG>(have ? g.x + g.y + g.z + g.w : 0.f) / E;
  const float mgx = group_sum<LG>(have ? g.x * xh.x + g.y * xh.y + g.z * xh.z + g.w * xh.w : 0.f) / E;
  if (have)
    store4(dx + row * E + 4 * lig,
           make_float4(rstd * (g.x - mg - xh.x * mgx), rstd * (g.y - mg - xh.y * mgx), rstd * (g.z - mg - xh.z * mgx),
                       rstd * (g.w - mg - xh.w * mgx)));
}

// fp32 backward: dx as above; also writes dy * xhat (its column sum is dw)
template <int LG>
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ w, const float* __restrict__ stats,
                                                            int64_t R, int E, float* __restrict__ dx,
                                                            float* __restrict__ dyxhat) {
  const int lig = threadIdx.x % LG;
  const bool live = lig * 4 < E;
  const float4 wv = live ? *reinterpret_cast<const float4*>(w + 4 * lig) : make_float4(0, 0, 0, 0);
  for (int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LG; row < R;
       row += ((int64_t)gridDim.x * blockDim.x) / LG) {
    float4 gy, xh;
    layernorm_bwd_row<LG, float>(dy, x, nullptr, wv, stats[2 * row], stats[2 * row + 1], row, E, lig, live, dx, gy, xh);
    if (live) store4(dyxhat + row * E + 4 * lig, make_float4(gy.x * xh.x, gy.y * xh.y, gy.z * xh.z, gy.w * xh.w));
  }
}

// The reference's other activations (code/layers.py:13-80 get_act: tanh, sigmoid, none, elu, leu, gelu (erf),
// gelu_new (tanh form), swish, mish; `hidden_act` of MLPBlock, layers.py:173-188) as one elementwise pass
// after the plain Linear (+ bias) GEMM, and dz = dy f'(z) recomputed from the saved pre-activation in backward.
// Not the benchmarked path (every DCNv2 script uses relu, which is fused into the GEMM epilogue): HBM-bound.
enum { kActTanh = 1, kActSigmoid, kActNone, kActElu, kActLeu, kActGelu, kActGeluNew, kActSwish, kActMish };

__device__ inline float act_value(int kind, float z) {
  switch (kind) {
    case kActTanh: return tanhf(z);
    case kActSigmoid: return 1.f / (1.f + expf(-z));
    case kActElu: return z > 0.f ? z : expm1f(z);
    case kActLeu: return z > 0.f ? logf(z + 1.f) : expf(z) - 1.f;                 // layers.py:22-27 (alpha = 1)
    case kActGelu: return z * 0.5f * (1.f + erff(z * 0.70710678118654752f));       // layers.py:36-37
    case kActGeluNew: {                                                            // layers.py:41-42
      const float u = 0.79788456080286536f * (z + 0.044715f * z * z * z);
      return 0.5f * z * (1.f + tanhf(u));
    }
    case kActSwish: return z / (1.f + expf(-z));                                   // layers.py:46-47
    case kActMish: {                                                               // layers.py:51-52
      const float sp = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
      return z * tanhf(sp);
    }
    default: return z;
  }
}

__device__ inline float act_slope(int kind, float z) {
  switch (kind) {
    case kActTanh: { const float t = tanhf(z); return 1.f - t * t; }
    case kActSigmoid: { const float s = 1.f / (1.f + expf(-z)); return s * (1.f - s); }
    case kActElu: return z > 0.f ? 1.f : expf(z);
    case kActLeu: return z > 0.f ? 1.f / (z + 1.f) : expf(z);
    case kActGelu:
      return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * expf(-0.5f * z * z);
    case kActGeluNew: {
      const float u = 0.79788456080286536f * (z + 0.044715f * z * z * z), t = tanhf(u);
      return 0.5f * (1.f + t) + 0.5f * z * (1.f - t * t) * 0.79788456080286536f * (1.f + 3.f * 0.044715f * z * z);
    }
    case kActSwish: { const float s = 1.f / (1.f + expf(-z)); return s + z * s * (1.f - s); }
    case kActMish: {
      const float sp = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))), t = tanhf(sp), s = 1.f / (1.f + expf(-z));
      return t + z * (1.f - t * t) * s;
    }
    default: return 1.f;
  }
}

// y[m, :] (row stride ldy) = f(z[m, :]);  dz = dy * f'(z)  (dy row stride ld_dy)
// T: float, or bf16_t (bf16 compute mode: the saved pre-activation z, y, dy and dz are bf16; f and f' in fp32, one
// rounding per store).  `vec` (bf16 only): N and the row strides are multiples of 4 and the bases 8-byte aligned, so
// a thread takes four elements of a row per load and store.
template <class T>
__global__ void __launch_bounds__(256) act_fwd_kernel(int kind, const T* __restrict__ z, int64_t M, int N,
                                                      T* __restrict__ y, int64_t ldy, int vec) {
  if constexpr (sizeof(T) == 2) {
    if (vec) {
      const int N4 = N / 4;
      for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * N4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / N4;
        const float4 v = load4(z + 4 * i);
        store4(y + m * ldy + 4 * (i - m * N4), make_float4(act_value(kind, v.x), act_value(kind, v.y),
                                                           act_value(kind, v.z), act_value(kind, v.w)));
      }
      return;
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * N; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / N;
    y[m * ldy + (i - m * N)] = (T)act_value(kind, (float)z[i]);
  }
}
template <class T>
__global__ void __launch_bounds__(256) act_bwd_kernel(int kind, const T* __restrict__ dy, int64_t ld_dy,
                                                      const T* __restrict__ z, int64_t M, int N,
                                                      T* __restrict__ dz, int vec) {
  if constexpr (sizeof(T) == 2) {
    if (vec) {
      const int N4 = N / 4;
      for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * N4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / N4;
        const float4 v = load4(z + 4 * i), g = load4(dy + m * ld_dy + 4 * (i - m * N4));
        store4(dz + 4 * i, make_float4(g.x * act_slope(kind, v.x), g.y * act_slope(kind, v.y),
                                       g.z * act_slope(kind, v.z), g.w * act_slope(kind, v.w)));
      }
      return;
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * N; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / N;
    dz[i] = (T)((float)dy[m * ld_dy + (i - m * N)] * act_slope(kind, (float)z[i]));
  }
}

// Backward of the bf16 add + LayerNorm: the sum is recomputed from x and s; dsum (layernorm_bwd_row's dv) is the
// gradient of BOTH addends (bf16, rounded once).  dL/dw = sum_rows dy * xhat and dL/db =
// sum_rows dy leave as ONE fp32 partial row per workgroup, part [gridDim.x, 2E] = (dw | db): a lane adds its rows'
// terms in row order, the wave's lanes of one column group are added by a fixed butterfly, the four waves in wave
// order — no [R, E] dy * xhat tensor, no atomics, bitwise deterministic.  The caller sums the rows (mapx_sum_tasks).
constexpr int kAddLnBwdMaxGroups = 512;      // 2 workgroups per CU keep HBM busy; 512 x 2E floats of partials

template <int LG>
__global__ void __launch_bounds__(256) add_layernorm_bwd_bf16_kernel(const bf16_t* __restrict__ dy,
                                                                     const bf16_t* __restrict__ x,
                                                                     const bf16_t* __restrict__ s,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ stats, int64_t R, int E,
                                                                     bf16_t* __restrict__ dsum,
                                                                     float* __restrict__ part) {
  __shared__ float4 red[2][4][LG];
  const int lig = threadIdx.x % LG;
  const bool live = lig * 4 < E;
  const float4 wv = live ? *reinterpret_cast<const float4*>(w + 4 * lig) : make_float4(0, 0, 0, 0);
  float4 aw = make_float4(0, 0, 0, 0), ab = make_float4(0, 0, 0, 0);
  // (every lane of a wave runs the same number of rounds: the group_sum shuffles need all 64 lanes)
  const int64_t stride = ((int64_t)gridDim.x * blockDim.x) / LG;
  for (int64_t r0 = ((int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~(kWave - 1))) / LG; r0 < R; r0 += stride) {
    const int64_t row = r0 + (threadIdx.x & (kWave - 1)) / LG;
    const bool have = live && row < R;
    const float mean = row < R ? stats[2 * row] : 0.f, rstd = row < R ? stats[2 * row + 1] : 0.f;
    float4 gy, xh;
    layernorm_bwd_row<LG>(dy, x, s, wv, mean, rstd, row, E, lig, have, dsum, gy, xh);
    if (have) {
      aw.x = fmaf(gy.x, xh.x, aw.x); aw.y = fmaf(gy.y, xh.y, aw.y);
      aw.z = fmaf(gy.z, xh.z, aw.z); aw.w = fmaf(gy.w, xh.w, aw.w);
      ab.x += gy.x; ab.y += gy.y; ab.z += gy.z; ab.w += gy.w;
    }
  }
#pragma unroll
  for (int o = LG; o < kWave; o <<= 1) {       // the wave's 64 / LG rows of one column group
    aw.x += __shfl_xor(aw.x, o, kWave); aw.y += __shfl_xor(aw.y, o, kWave);
    aw.z += __shfl_xor(aw.z, o, kWave); aw.w += __shfl_xor(aw.w, o, kWave);
    ab.x += __shfl_xor(ab.x, o, kWave); ab.y += __shfl_xor(ab.y, o, kWave);
    ab.z += __shfl_xor(ab.z, o, kWave); ab.w += __shfl_xor(ab.w, o, kWave);
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane < LG) {
    red[0][wave][lane] = aw;
    red[1][wave][lane] = ab;
  }
  __syncthreads();
  if (threadIdx.x < LG && live) {
    float4 tw = red[0][0][lig], tb = red[1][0][lig];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float4 a = red[0][k][lig], c = red[1][k][lig];
      tw.x += a.x; tw.y += a.y; tw.z += a.z; tw.w += a.w;
      tb.x += c.x; tb.y += c.y; tb.z += c.z; tb.w += c.w;
    }
    float* prow = part + (int64_t)blockIdx.x * 2 * E;
    *reinterpret_cast<float4*>(prow + 4 * lig) = tw;
    *reinterpret_cast<float4*>(prow + E + 4 * lig) = tb;
  }
}

static int ln_lanes(int E) { return E <= 16 ? 4 : (E <= 32 ? 8 : 16); }
static int add_ln_bwd_groups(int64_t R, int E) { return grid_for(R * ln_lanes(E), 256, kAddLnBwdMaxGroups); }

template <class T>
static int layernorm_fwd_launch(const char* what, const T* x, const T* s_opt, int64_t R, int E, const float* w,
                                const float* b, float eps, T* y, float* stats, hipStream_t stream) {
  const int lg = ln_lanes(E);
  const int grid = grid_for(R * lg, 256);
  if (lg == 4)
    hipLaunchKernelGGL((layernorm_fwd_kernel<4, T>), dim3(grid), dim3(256), 0, stream, x, s_opt, R, E, w, b, eps, y, stats);
  else if (lg == 8)
    hipLaunchKernelGGL((layernorm_fwd_kernel<8, T>), dim3(grid), dim3(256), 0, stream, x, s_opt, R, E, w, b, eps, y, stats);
  else
    hipLaunchKernelGGL((layernorm_fwd_kernel<16, T>), dim3(grid), dim3(256), 0, stream, x, s_opt, R, E, w, b, eps, y, stats);
  return check_launch(what);
}

}  // namespace mapx

extern "C" int mapx_dropout(const float* x, int64_t n, float p, uint64_t seed, uint64_t offset,
                            const int32_t* offset_dev, float* out, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 0 && p >= 0.f && p < 1.f, "dropout: bad arguments (0 <= p < 1)");
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(x && out, "dropout: null pointer");
  hipLaunchKernelGGL(dropout_kernel<float>, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, stream, x, n, p,
                     1.f / (1.f - p), seed, offset, offset_dev, out, 0);
  return check_launch("dropout");
}

extern "C" int mapx_dropout_bf16(const mapx_bf16* x, int64_t n, float p, uint64_t seed, uint64_t offset,
                                 const int32_t* offset_dev, mapx_bf16* out, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 0 && p >= 0.f && p < 1.f, "dropout_bf16: bad arguments (0 <= p < 1)");
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(x && out, "dropout_bf16: null pointer");
  const int vec = ((uintptr_t)x | (uintptr_t)out) % 8 == 0;
  hipLaunchKernelGGL(dropout_kernel<bf16_t>, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, stream, hc(x), n, p,
                     1.f / (1.f - p), seed, offset, offset_dev, hm(out), vec);
  return check_launch("dropout_bf16");
}

extern "C" int mapx_add_layernorm_fwd_bf16(const mapx_bf16* x, const mapx_bf16* s_opt, int64_t R, int E, const float* w,
                                           const float* b, float eps, mapx_bf16* y, float* stats, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(R >= 0 && E >= 4 && E <= 64 && E % 4 == 0, "add_layernorm_fwd_bf16: E must be a multiple of 4 in [4, 64]");
  if (R == 0) return MAPX_OK;
  MAPX_REQUIRE(x && w && b && y && stats, "add_layernorm_fwd_bf16: null pointer");
  MAPX_REQUIRE(((uintptr_t)x | (uintptr_t)s_opt | (uintptr_t)y) % 8 == 0 && ((uintptr_t)w | (uintptr_t)b) % 16 == 0,
               "add_layernorm_fwd_bf16: x, s, y must be 8-byte aligned, w and b 16-byte aligned");
  return layernorm_fwd_launch("add_layernorm_fwd_bf16", hc(x), hc(s_opt), R, E, w, b, eps, hm(y), stats, stream);
}

extern "C" int mapx_add_layernorm_bwd_groups(int64_t R, int E) {
  return (R >= 1 && E >= 4 && E <= 64) ? mapx::add_ln_bwd_groups(R, E) : 0;
}

extern "C" int mapx_add_layernorm_bwd_bf16(const mapx_bf16* dy, const mapx_bf16* x, const mapx_bf16* s_opt,
                                           const float* w, const float* stats, int64_t R, int E, mapx_bf16* dsum,
                                           float* part, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(R >= 0 && E >= 4 && E <= 64 && E % 4 == 0, "add_layernorm_bwd_bf16: E must be a multiple of 4 in [4, 64]");
  if (R == 0) return MAPX_OK;
  MAPX_REQUIRE(dy && x && w && stats && dsum && part, "add_layernorm_bwd_bf16: null pointer");
  MAPX_REQUIRE(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)s_opt | (uintptr_t)dsum) % 8 == 0 &&
                   ((uintptr_t)w | (uintptr_t)part) % 16 == 0,
               "add_layernorm_bwd_bf16: dy, x, s, dsum must be 8-byte aligned, w and part 16-byte aligned");
  const int lg = ln_lanes(E);
  const int grid = add_ln_bwd_groups(R, E);
#define MAPX_ADD_LN_BWD(LG)                                                                                        \
  hipLaunchKernelGGL(add_layernorm_bwd_bf16_kernel<LG>, dim3(grid), dim3(256), 0, stream, hc(dy), hc(x), hc(s_opt), w, \
                     stats, R, E, hm(dsum), part)
  if (lg == 4) MAPX_ADD_LN_BWD(4);
  else if (lg == 8) MAPX_ADD_LN_BWD(8);
  else MAPX_ADD_LN_BWD(16);
#undef MAPX_ADD_LN_BWD
  return check_launch("add_layernorm_bwd_bf16");
}

extern "C" int mapx_layernorm_fwd(const float* x, int64_t R, int E, const float* w, const float* b, float eps, float* y,
                                  float* stats, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(R >= 0 && E >= 4 && E <= 64 && E % 4 == 0, "layernorm_fwd: E must be a multiple of 4 in [4, 64]");
  if (R == 0) return MAPX_OK;
  MAPX_REQUIRE(x && w && b && y && stats, "layernorm_fwd: null pointer");
  return layernorm_fwd_launch<float>("layernorm_fwd", x, nullptr, R, E, w, b, eps, y, stats, stream);
}

extern "C" int mapx_layernorm_bwd(const float* dy, const float* x, const float* w, const float* stats, int64_t R, int E,
                                  float* dx, float* dy_xhat, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(R >= 0 && E >= 4 && E <= 64 && E % 4 == 0, "layernorm_bwd: E must be a multiple of 4 in [4, 64]");
  if (R == 0) return MAPX_OK;
  MAPX_REQUIRE(dy && x && w && stats && dx && dy_xhat, "layernorm_bwd: null pointer");
  const int lg = ln_lanes(E);
  const int grid = grid_for(R * lg, 256);
  if (lg == 4) hipLaunchKernelGGL(layernorm_bwd_kernel<4>, dim3(grid), dim3(256), 0, stream, dy, x, w, stats, R, E, dx, dy_xhat);
  else if (lg == 8) hipLaunchKernelGGL(layernorm_bwd_kernel<8>, dim3(grid), dim3(256), 0, stream, dy, x, w, stats, R, E, dx, dy_xhat);
  else hipLaunchKernelGGL(layernorm_bwd_kernel<16>, dim3(grid), dim3(256), 0, stream, dy, x, w, stats, R, E, dx, dy_xhat);
  return check_launch("layernorm_bwd");
}

extern "C" int mapx_act_fwd(int kind, const float* z, int64_t M, int N, float* y, int64_t ldy, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(kind >= kActTanh && kind <= kActMish, "act_fwd: unknown activation %d", kind);
  MAPX_REQUIRE(M >= 0 && N > 0 && ldy >= N, "act_fwd: bad sizes");
  if (M == 0) return MAPX_OK;
  MAPX_REQUIRE(z && y, "act_fwd: null pointer");
  hipLaunchKernelGGL(act_fwd_kernel<float>, dim3(grid_for(M * N, 256)), dim3(256), 0, stream, kind, z, M, N, y, ldy, 0);
  return check_launch("act_fwd");
}

extern "C" int mapx_act_fwd_bf16(int kind, const mapx_bf16* z, int64_t M, int N, mapx_bf16* y, int64_t ldy,
                                 hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(kind >= kActTanh && kind <= kActMish, "act_fwd_bf16: unknown activation %d", kind);
  MAPX_REQUIRE(M >= 0 && N > 0 && ldy >= N, "act_fwd_bf16: bad sizes");
  if (M == 0) return MAPX_OK;
  MAPX_REQUIRE(z && y, "act_fwd_bf16: null pointer");
  const int vec = N % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)z | (uintptr_t)y) % 8 == 0;
  hipLaunchKernelGGL(act_fwd_kernel<bf16_t>, dim3(grid_for(vec ? M * (N / 4) : M * N, 256)), dim3(256), 0, stream, kind,
                     hc(z), M, N, hm(y), ldy, vec);
  return check_launch("act_fwd_bf16");
}

extern "C" int mapx_act_bwd(int kind, const float* dy, int64_t ld_dy, const float* z, int64_t M, int N, float* dz,
                            hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(kind >= kActTanh && kind <= kActMish, "act_bwd: unknown activation %d", kind);
  MAPX_REQUIRE(M >= 0 && N > 0 && ld_dy >= N, "act_bwd: bad sizes");
  if (M == 0) return MAPX_OK;
  MAPX_REQUIRE(dy && z && dz, "act_bwd: null pointer");
  hipLaunchKernelGGL(act_bwd_kernel<float>, dim3(grid_for(M * N, 256)), dim3(256), 0, stream, kind, dy, ld_dy, z, M, N,
                     dz, 0);
  return check_launch("act_bwd");
}

extern "C" int mapx_act_bwd_bf16(int kind, const mapx_bf16* dy, int64_t ld_dy, const mapx_bf16* z, int64_t M, int N,
                                 mapx_bf16* dz, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(kind >= kActTanh && kind <= kActMish, "act_bwd_bf16: unknown activation %d", kind);
  MAPX_REQUIRE(M >= 0 && N > 0 && ld_dy >= N, "act_bwd_bf16: bad sizes");
  if (M == 0) return MAPX_OK;
  MAPX_REQUIRE(dy && z && dz, "act_bwd_bf16: null pointer");
  const int vec = N % 4 == 0 && ld_dy % 4 == 0 && ((uintptr_t)dy | (uintptr_t)z | (uintptr_t)dz) % 8 == 0;
  hipLaunchKernelGGL(act_bwd_kernel<bf16_t>, dim3(grid_for(vec ? M * (N / 4) : M * N, 256)), dim3(256), 0, stream, kind,
                     hc(dy), ld_dy, hc(z), M, N, hm(dz), vec);
  return check_launch("act_bwd_bf16");
}
