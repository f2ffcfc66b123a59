// Self-attention core of the Transformer backbone (reference code/models.py:491-568: nn.TransformerEncoderLayer's
// nn.MultiheadAttention, batch_first) on field-sized sequences, and the field pooling of its finetune head.
//
// Attention.  qkv [M = B*F, 3E] is the in-projection's output as it stands: row b*F + f, columns [0,E) = Q,
// [E,2E) = K, [2E,3E) = V; head h owns columns [h*dh, (h+1)*dh) of each third (dh = E/H).  Per group g = b*H + h:
//   P = softmax(Q K^T / sqrt(dh)) [F,F] (kept, undropped, for backward);  P~ = P * m / (1-p);  O = P~ V,
// O written into o [M, E] at the same columns of the head: the head-concatenated layout out_proj reads.  The keep
// mask m is regenerated from Philox in backward (mha_keep4: one dropout draw of common.h per 4 keys of a query row),
// never stored.
//
// Layout (attn.hip's): one wave per group, Q/K/V rows in LDS (16-byte rows, float4 loads along dh), one lane per
// query row, two groups per wave when F <= 32.  The F x F probabilities live in LDS at a row pitch of F+1 floats
// (lane i walks row i: conflict-free).  The work is tiny and HBM-bound: qkv in, O and P out.
//
// Element type T of qkv, o, d_o and d_qkv (and of the pooling's x, out, g, dx): float, or bf16_t in bf16 compute mode
// (DESIGN §4.6).  Only the global loads and stores differ (common.h load4 / store4): a load widens into the same fp32
// LDS rows, the arithmetic is the fp32 code, a store rounds once.  P, the pooling weights and d_scores are fp32 for
// both.  A head's row section starts at a multiple of 4 elements and is a multiple of 4 wide, so the four-element
// accesses are 8-byte aligned in bf16 as they are 16-byte aligned in fp32.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr int kMhaMaxF = 64, kMhaMaxDh = 64;

// Keep bits of keys 4q .. 4q+3 of query row `row` (= g*F + i) of the probability matrices: bit e set = key 4q+e
// kept.  The counter of the attention-dropout mask (the draw itself: common.h): both kernels and
// mapx_mha_dropout_mask call it.  attn.hip's P mask uses the same counter.
__device__ inline uint32_t mha_keep4(uint64_t seed, uint64_t off, uint32_t thr, int64_t row, int nq4, int q) {
  return keep_bits4(philox4x32_10(seed, (uint64_t)(row * nq4 + q), off), thr);
}

// Cooperative 16-byte loads of `nsec` row sections of width dh (each starting at column col0 + s*E of the rows
// b*F .. b*F+F-1, row pitch ld elements) into LDS at [s][r][LD].
template <class T>
__device__ inline void load_sections(const T* __restrict__ src, int64_t ld, int64_t row0, int col0, int E,
                                     int nsec, int F, int dh, int LD, float* dst, int li, int LW) {
  const int dh4 = dh / 4;
  const int n = nsec * F * dh4;
  for (int t = li; t < n; t += LW) {
    const int c = t % dh4, rs = t / dh4, r = rs % F, s = rs / F;
    const float4 v = load4(src + (row0 + r) * ld + col0 + s * E + 4 * c);
    *reinterpret_cast<float4*>(dst + (s * F + r) * LD + 4 * c) = v;
  }
}

// DHB: dh rounded up to a bucket (registers hold one row of dh floats); GPW groups per wave.
template <int GPW, int DHB, class T>
__global__ void __launch_bounds__(64) mha_fwd_kernel(const T* __restrict__ qkv, int64_t G, int H, int F, int E,
                                                     float scale, float p, uint64_t seed, uint64_t offset,
                                                     const int32_t* __restrict__ offset_dev, T* __restrict__ o,
                                                     float* __restrict__ probs) {
  extern __shared__ float4 sm4[];
  float* sm = reinterpret_cast<float*>(sm4);
  constexpr int LW = 64 / GPW, C4 = DHB / 4;
  const int dh = E / H, dh4 = dh / 4, LD = dh + 4, LF = F + 1;
  const int half = threadIdx.x / LW, li = threadIdx.x % LW;
  float* Qs = sm + half * ((3 * F * LD + F * LF + 3) & ~3);     // Q, K, V [F][LD]; P [F][LF]
  float* Ks = Qs + F * LD;
  float* Vs = Ks + F * LD;
  float* Ps = Vs + F * LD;
  const int64_t g = (int64_t)blockIdx.x * GPW + half;
  const bool have = g < G;
  const int64_t b = have ? g / H : 0;
  const int h = have ? (int)(g - b * H) : 0;
  const int64_t row0 = b * F;
  if (have) load_sections(qkv, 3 * (int64_t)E, row0, h * dh, E, 3, F, dh, LD, Qs, li, LW);
  __syncthreads();
  const int i = li;
  if (have && i < F) {
    float4 q[C4];
#pragma unroll
    for (int c = 0; c < C4; ++c)
      q[c] = c < dh4 ? *reinterpret_cast<const float4*>(Qs + i * LD + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    float mx = -3.4e38f;
    for (int j = 0; j < F; ++j) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < C4; ++c)
        if (c < dh4) s = dot4(q[c], *reinterpret_cast<const float4*>(Ks + j * LD + 4 * c), s);
      s *= scale;
      Ps[i * LF + j] = s;
      mx = fmaxf(mx, s);
    }
    float den = 0.f;
    for (int j = 0; j < F; ++j) {
      const float e = expf(Ps[i * LF + j] - mx);
      Ps[i * LF + j] = e;
      den += e;
    }
    const float rden = 1.f / den;
    float4 acc[C4];
#pragma unroll
    for (int c = 0; c < C4; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool drop = p > 0.f;
    const uint32_t thr = drop_threshold(p);
    const uint64_t off = drop ? drop_offset(offset, offset_dev) : 0;
    const float rkeep = drop ? 1.f / (1.f - p) : 1.f;
    const int nq4 = (F + 3) / 4;
    uint32_t keep = 0xFu;
    for (int j = 0; j < F; ++j) {
      const float pij = Ps[i * LF + j] * rden;
      Ps[i * LF + j] = pij;
      if (drop && (j & 3) == 0) keep = mha_keep4(seed, off, thr, g * F + i, nq4, j >> 2);
      const float pd = drop ? (((keep >> (j & 3)) & 1u) ? pij * rkeep : 0.f) : pij;
#pragma unroll
      for (int c = 0; c < C4; ++c)
        if (c < dh4) fma4(acc[c], pd, *reinterpret_cast<const float4*>(Vs + j * LD + 4 * c));
    }
    T* orow = o + (row0 + i) * E + h * dh;
#pragma unroll
    for (int c = 0; c < C4; ++c)
      if (c < dh4) store4(orow + 4 * c, acc[c]);
  }
  __syncthreads();
  for (int t = li; have && t < F * F; t += LW) {       // coalesced copy of the probabilities for backward
    const int r = t / F, c = t - r * F;
    probs[g * F * F + t] = Ps[r * LF + c];
  }
}

// dV = P~^T dO;  dP = (dO V^T) m / (1-p);  dS = P (dP - rowsum(P dP)) scale;  dQ = dS K;  dK = dS^T Q
template <int GPW, int DHB, class T>
__global__ void __launch_bounds__(64) mha_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ probs,
                                                     const T* __restrict__ d_o, int64_t G, int H, int F, int E,
                                                     float scale, float p, uint64_t seed, uint64_t offset,
                                                     const int32_t* __restrict__ offset_dev,
                                                     T* __restrict__ d_qkv) {
  extern __shared__ float4 sm4[];
  float* sm = reinterpret_cast<float*>(sm4);
  constexpr int LW = 64 / GPW, C4 = DHB / 4;
  const int dh = E / H, dh4 = dh / 4, LD = dh + 4, LF = F + 1;
  const int half = threadIdx.x / LW, li = threadIdx.x % LW;
  float* Qs = sm + half * ((4 * F * LD + 2 * F * LF + 3) & ~3);   // Q, K, V, dO [F][LD]; P (then P~), dS [F][LF]
  float* Ks = Qs + F * LD;
  float* Vs = Ks + F * LD;
  float* Ds = Vs + F * LD;
  float* Ps = Ds + F * LD;
  float* dS = Ps + F * LF;
  const int64_t g = (int64_t)blockIdx.x * GPW + half;
  const bool have = g < G;
  const int64_t b = have ? g / H : 0;
  const int h = have ? (int)(g - b * H) : 0;
  const int64_t row0 = b * F;
  if (have) {
    load_sections(qkv, 3 * (int64_t)E, row0, h * dh, E, 3, F, dh, LD, Qs, li, LW);
    load_sections(d_o, E, row0, h * dh, E, 1, F, dh, LD, Ds, li, LW);
    for (int t = li; t < F * F; t += LW) {
      const int r = t / F, c = t - r * F;
      Ps[r * LF + c] = probs[g * F * F + t];
    }
  }
  __syncthreads();
  const int i = li;
  const int ldq = 3 * E;
  if (have && i < F) {
    float4 dov[C4];
#pragma unroll
    for (int c = 0; c < C4; ++c)
      dov[c] = c < dh4 ? *reinterpret_cast<const float4*>(Ds + i * LD + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool drop = p > 0.f;
    const uint32_t thr = drop_threshold(p);
    const uint64_t off = drop ? drop_offset(offset, offset_dev) : 0;
    const float rkeep = drop ? 1.f / (1.f - p) : 1.f;
    const int nq4 = (F + 3) / 4;
    uint32_t keep = 0xFu;
    float dot = 0.f;
    for (int j = 0; j < F; ++j) {
      float dp = 0.f;
#pragma unroll
      for (int c = 0; c < C4; ++c)
        if (c < dh4) dp = dot4(dov[c], *reinterpret_cast<const float4*>(Vs + j * LD + 4 * c), dp);
      const float pij = Ps[i * LF + j];
      if (drop) {
        if ((j & 3) == 0) keep = mha_keep4(seed, off, thr, g * F + i, nq4, j >> 2);
        const bool k = (keep >> (j & 3)) & 1u;
        dp = k ? dp * rkeep : 0.f;
        Ps[i * LF + j] = k ? pij * rkeep : 0.f;          // P~ for dV below
      }
      dS[i * LF + j] = dp;
      dot = fmaf(pij, dp, dot);
    }
    float4 acc[C4];
#pragma unroll
    for (int c = 0; c < C4; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    // P itself (needed for dS) is read back from global: with dropout the LDS copy now holds P~
    const float* prow = probs + (g * F + i) * F;
    for (int j = 0; j < F; ++j) {
      const float pij = drop ? prow[j] : Ps[i * LF + j];
      const float ds = pij * (dS[i * LF + j] - dot) * scale;
      dS[i * LF + j] = ds;
#pragma unroll
      for (int c = 0; c < C4; ++c)
        if (c < dh4) fma4(acc[c], ds, *reinterpret_cast<const float4*>(Ks + j * LD + 4 * c));
    }
    T* dq = d_qkv + (row0 + i) * ldq + h * dh;
#pragma unroll
    for (int c = 0; c < C4; ++c)
      if (c < dh4) store4(dq + 4 * c, acc[c]);
  }
  __syncthreads();
  if (have && i < F) {                           // lane i now owns key / value row i: sums over the query rows
    float4 ak[C4], av[C4];
#pragma unroll
    for (int c = 0; c < C4; ++c) ak[c] = av[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = 0; r < F; ++r) {
      const float ds = dS[r * LF + i], pd = Ps[r * LF + i];
#pragma unroll
      for (int c = 0; c < C4; ++c)
        if (c < dh4) {
          fma4(ak[c], ds, *reinterpret_cast<const float4*>(Qs + r * LD + 4 * c));
          fma4(av[c], pd, *reinterpret_cast<const float4*>(Ds + r * LD + 4 * c));
        }
    }
    T* dk = d_qkv + (row0 + i) * ldq + E + h * dh;
    T* dv = dk + E;
#pragma unroll
    for (int c = 0; c < C4; ++c)
      if (c < dh4) {
        store4(dk + 4 * c, ak[c]);
        store4(dv + 4 * c, av[c]);
      }
  }
}

__global__ void __launch_bounds__(256) mha_mask_kernel(int64_t rows, int F, float p, uint64_t seed, uint64_t offset,
                                                       const int32_t* __restrict__ offset_dev,
                                                       uint8_t* __restrict__ keep) {
  const uint64_t off = drop_offset(offset, offset_dev);
  const uint32_t thr = drop_threshold(p);
  const int nq4 = (F + 3) / 4;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * nq4; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / nq4;
    const int q = (int)(t - row * nq4);
    const uint32_t k = mha_keep4(seed, off, thr, row, nq4, q);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < F) keep[row * F + 4 * q + e] = (uint8_t)((k >> e) & 1u);
  }
}

// ---------------------------------------------------------------- field pooling of the finetune head
// x [B,F,E] -> out [B,E]: mode 0 sum_f x, 1 (sum_f x) / F, 2 sum_f w_f x with w = softmax_f(scores [B,F]) (w kept
// for backward).  16 lanes per sample, float4 columns.
constexpr int kPoolLanes = 16;

// Softmax over the F scores of a sample: every lane of the sample computes (max, 1 / denominator) itself, so no lane
// waits for another; the weights are w_f = exp(s_f - max) / den as nn.Softmax forms them.
__device__ inline void pool_softmax_stats(const float* __restrict__ s, int F, float& mx, float& den) {
  mx = -3.4e38f;
  for (int f = 0; f < F; ++f) mx = fmaxf(mx, s[f]);
  den = 0.f;
  for (int f = 0; f < F; ++f) den += expf(s[f] - mx);
}

template <class T>
__global__ void __launch_bounds__(256) field_pool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ scores,
                                                             int64_t B, int F, int E, int mode,
                                                             T* __restrict__ out, float* __restrict__ w) {
  const int lane = threadIdx.x % kPoolLanes;
  const int E4 = E / 4;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kPoolLanes; b < B;
       b += ((int64_t)gridDim.x * blockDim.x) / kPoolLanes) {
    float mx = 0.f, den = 1.f;
    if (mode == 2) {
      pool_softmax_stats(scores + b * F, F, mx, den);
      for (int f = lane; f < F; f += kPoolLanes) w[b * F + f] = expf(scores[b * F + f] - mx) / den;
    }
    for (int c = lane; c < E4; c += kPoolLanes) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int f = 0; f < F; ++f) {
        const float4 v = load4(x + (b * F + f) * E + 4 * c);
        if (mode == 2) fma4(acc, expf(scores[b * F + f] - mx) / den, v);
        else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
      }
      if (mode == 1) acc = make_float4(acc.x / F, acc.y / F, acc.z / F, acc.w / F);
      store4(out + b * E + 4 * c, acc);
    }
  }
}

// dx[b,f,:] = w_f g[b,:] (sum: w_f = 1, mean: 1/F);  attn: d_scores[b,f] = w_f (g.x_f - sum_k w_k g.x_k)
template <class T>
__global__ void __launch_bounds__(256) field_pool_bwd_kernel(const T* __restrict__ g, const T* __restrict__ x,
                                                             const float* __restrict__ w, int64_t B, int F, int E,
                                                             int mode, T* __restrict__ dx,
                                                             float* __restrict__ d_scores) {
  const int lane = threadIdx.x % kPoolLanes;
  const int E4 = E / 4;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kPoolLanes; b < B;
       b += ((int64_t)gridDim.x * blockDim.x) / kPoolLanes) {
    float tot = 0.f;
    for (int f = 0; f < F; ++f) {
      const float wf = mode == 2 ? w[b * F + f] : (mode == 1 ? 1.f / F : 1.f);
      float gx = 0.f;
      for (int c = lane; c < E4; c += kPoolLanes) {
        const float4 gv = load4(g + b * E + 4 * c);
        if (mode == 2) gx = dot4(gv, load4(x + (b * F + f) * E + 4 * c), gx);
        if (mode == 1) store4(dx + (b * F + f) * E + 4 * c, make_float4(gv.x / F, gv.y / F, gv.z / F, gv.w / F));
        else store4(dx + (b * F + f) * E + 4 * c, make_float4(wf * gv.x, wf * gv.y, wf * gv.z, wf * gv.w));
      }
      if (mode == 2) {
        gx = group_sum<kPoolLanes>(gx);
        tot = fmaf(wf, gx, tot);
      }
    }
    if (mode == 2) {
      for (int f = lane; f < F; f += kPoolLanes) {
        float gx = 0.f;
        for (int c = 0; c < E4; ++c)
          gx = dot4(load4(g + b * E + 4 * c), load4(x + (b * F + f) * E + 4 * c), gx);
        d_scores[b * F + f] = w[b * F + f] * (gx - tot);
      }
    }
  }
}

// F = dh = 64 needs 104 KB of dynamic LDS in backward: above the 64 KB default, inside the CU's 160 KB
template <int GPW, class T>
static hipError_t mha_allow_lds() {
  static const hipError_t done = allow_dynamic_lds(
      128 * 1024, &mha_fwd_kernel<GPW, 8, T>, &mha_fwd_kernel<GPW, 16, T>, &mha_fwd_kernel<GPW, 32, T>,
      &mha_fwd_kernel<GPW, 64, T>, &mha_bwd_kernel<GPW, 8, T>, &mha_bwd_kernel<GPW, 16, T>, &mha_bwd_kernel<GPW, 32, T>,
      &mha_bwd_kernel<GPW, 64, T>);
  return done;
}

static size_t mha_lds_bytes(int F, int dh, bool bwd) {
  const size_t LD = dh + 4, LF = F + 1;
  return (((bwd ? 4 * F * LD + 2 * F * LF : 3 * F * LD + F * LF) + 3) & ~(size_t)3) * sizeof(float);   // 16-byte groups
}

static int mha_check(const char* what, int64_t B, int F, int E, int H, float p) {
  MAPX_REQUIRE(B >= 0 && F >= 1 && F <= kMhaMaxF && H >= 1 && E >= 4 && E % H == 0 && (E / H) % 4 == 0 &&
                   E / H <= kMhaMaxDh && p >= 0.f && p < 1.f,
               "%s: F <= %d fields, head size E/H a multiple of 4 and <= %d, 0 <= p < 1 (got F=%d E=%d H=%d p=%g)",
               what, kMhaMaxF, kMhaMaxDh, F, E, H, (double)p);
  return MAPX_OK;
}

static int dh_bucket(int dh) { return dh <= 8 ? 8 : (dh <= 16 ? 16 : (dh <= 32 ? 32 : 64)); }

#define MAPX_MHA_DISPATCH(KERNEL, GPW, GRID, LDS, ...)                                                     \
  switch (dh_bucket(E / H)) {                                                                              \
    case 8: hipLaunchKernelGGL((KERNEL<GPW, 8, T>), GRID, dim3(64), LDS, stream, __VA_ARGS__); break;      \
    case 16: hipLaunchKernelGGL((KERNEL<GPW, 16, T>), GRID, dim3(64), LDS, stream, __VA_ARGS__); break;    \
    case 32: hipLaunchKernelGGL((KERNEL<GPW, 32, T>), GRID, dim3(64), LDS, stream, __VA_ARGS__); break;    \
    default: hipLaunchKernelGGL((KERNEL<GPW, 64, T>), GRID, dim3(64), LDS, stream, __VA_ARGS__); break;    \
  }

template <class T>
static int mha_fwd_launch(const char* what, const T* qkv, int64_t B, int F, int E, int H, float p, uint64_t seed,
                          uint64_t offset, const int32_t* offset_dev_opt, T* o, float* probs, hipStream_t stream) {
  if (int st = mha_check(what, B, F, E, H, p)) return st;
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(qkv && o && probs, "%s: null pointer", what);
  MAPX_REQUIRE(((uintptr_t)qkv | (uintptr_t)o) % 16 == 0, "%s: qkv and o must be 16-byte aligned", what);
  const int64_t G = B * H;
  const float scale = 1.0f / sqrtf((float)(E / H));
  const size_t lds = mha_lds_bytes(F, E / H, false);
  if (F <= 32) {
    MAPX_HIP((mha_allow_lds<2, T>()));
    MAPX_MHA_DISPATCH(mha_fwd_kernel, 2, dim3((unsigned)((G + 1) / 2)), 2 * lds, qkv, G, H, F, E, scale, p, seed, offset,
                      offset_dev_opt, o, probs)
  } else {
    MAPX_HIP((mha_allow_lds<1, T>()));
    MAPX_MHA_DISPATCH(mha_fwd_kernel, 1, dim3((unsigned)G), lds, qkv, G, H, F, E, scale, p, seed, offset, offset_dev_opt,
                      o, probs)
  }
  return check_launch(what);
}

template <class T>
static int mha_bwd_launch(const char* what, const T* qkv, const float* probs, const T* d_o, int64_t B, int F, int E,
                          int H, float p, uint64_t seed, uint64_t offset, const int32_t* offset_dev_opt, T* d_qkv,
                          hipStream_t stream) {
  if (int st = mha_check(what, B, F, E, H, p)) return st;
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(qkv && probs && d_o && d_qkv, "%s: null pointer", what);
  MAPX_REQUIRE(((uintptr_t)qkv | (uintptr_t)d_o | (uintptr_t)d_qkv) % 16 == 0,
               "%s: qkv, d_o and d_qkv must be 16-byte aligned", what);
  const int64_t G = B * H;
  const float scale = 1.0f / sqrtf((float)(E / H));
  const size_t lds = mha_lds_bytes(F, E / H, true);
  if (F <= 32) {
    MAPX_HIP((mha_allow_lds<2, T>()));
    MAPX_MHA_DISPATCH(mha_bwd_kernel, 2, dim3((unsigned)((G + 1) / 2)), 2 * lds, qkv, probs, d_o, G, H, F, E, scale, p,
                      seed, offset, offset_dev_opt, d_qkv)
  } else {
    MAPX_HIP((mha_allow_lds<1, T>()));
    MAPX_MHA_DISPATCH(mha_bwd_kernel, 1, dim3((unsigned)G), lds, qkv, probs, d_o, G, H, F, E, scale, p, seed, offset,
                      offset_dev_opt, d_qkv)
  }
  return check_launch(what);
}
#undef MAPX_MHA_DISPATCH

template <class T>
static int field_pool_fwd_launch(const char* what, const T* x, const float* scores_opt, int64_t B, int F, int E,
                                 int mode, T* out, float* weights_opt, hipStream_t stream) {
  MAPX_REQUIRE(B >= 0 && F >= 1 && E >= 4 && E % 4 == 0 && mode >= 0 && mode <= 2,
               "%s: E a multiple of 4, mode 0 (sum) / 1 (mean) / 2 (softmax-weighted)", what);
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(x && out && (mode != 2 || (scores_opt && weights_opt)), "%s: null pointer", what);
  MAPX_REQUIRE(sizeof(T) == 4 || ((uintptr_t)x | (uintptr_t)out) % 8 == 0, "%s: x and out must be 8-byte aligned", what);
  hipLaunchKernelGGL(field_pool_fwd_kernel<T>, dim3(grid_for(B * kPoolLanes, 256)), dim3(256), 0, stream, x, scores_opt,
                     B, F, E, mode, out, weights_opt);
  return check_launch(what);
}

template <class T>
static int field_pool_bwd_launch(const char* what, const T* g, const T* x, const float* weights_opt, int64_t B, int F,
                                 int E, int mode, T* dx, float* d_scores_opt, hipStream_t stream) {
  MAPX_REQUIRE(B >= 0 && F >= 1 && E >= 4 && E % 4 == 0 && mode >= 0 && mode <= 2, "%s: bad arguments", what);
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(g && dx && (mode != 2 || (x && weights_opt && d_scores_opt)), "%s: null pointer", what);
  MAPX_REQUIRE(sizeof(T) == 4 || ((uintptr_t)g | (uintptr_t)x | (uintptr_t)dx) % 8 == 0,
               "%s: g, x and dx must be 8-byte aligned", what);
  hipLaunchKernelGGL(field_pool_bwd_kernel<T>, dim3(grid_for(B * kPoolLanes, 256)), dim3(256), 0, stream, g, x,
                     weights_opt, B, F, E, mode, dx, d_scores_opt);
  return check_launch(what);
}

}  // namespace mapx

extern "C" int mapx_mha_fwd(const float* qkv, int64_t B, int F, int E, int H, float p, uint64_t seed, uint64_t offset,
                            const int32_t* offset_dev_opt, float* o, float* probs, hipStream_t stream) {
  return mapx::mha_fwd_launch<float>("mha_fwd", qkv, B, F, E, H, p, seed, offset, offset_dev_opt, o, probs, stream);
}

extern "C" int mapx_mha_bwd(const float* qkv, const float* probs, const float* d_o, int64_t B, int F, int E, int H,
                            float p, uint64_t seed, uint64_t offset, const int32_t* offset_dev_opt, float* d_qkv,
                            hipStream_t stream) {
  return mapx::mha_bwd_launch<float>("mha_bwd", qkv, probs, d_o, B, F, E, H, p, seed, offset, offset_dev_opt, d_qkv,
                                     stream);
}

// bf16 I/O forms: the same kernel templates on bf16 elements (qkv, d_o in; o, d_qkv out); probs stays fp32.
extern "C" int mapx_mha_fwd_bf16(const mapx_bf16* qkv, int64_t B, int F, int E, int H, float p, uint64_t seed,
                                 uint64_t offset, const int32_t* offset_dev_opt, mapx_bf16* o, float* probs,
                                 hipStream_t stream) {
  using namespace mapx;
  return mha_fwd_launch<bf16_t>("mha_fwd_bf16", hc(qkv), B, F, E, H, p, seed, offset, offset_dev_opt, hm(o), probs,
                                stream);
}

extern "C" int mapx_mha_bwd_bf16(const mapx_bf16* qkv, const float* probs, const mapx_bf16* d_o, int64_t B, int F, int E,
                                 int H, float p, uint64_t seed, uint64_t offset, const int32_t* offset_dev_opt,
                                 mapx_bf16* d_qkv, hipStream_t stream) {
  using namespace mapx;
  return mha_bwd_launch<bf16_t>("mha_bwd_bf16", hc(qkv), probs, hc(d_o), B, F, E, H, p, seed, offset, offset_dev_opt,
                                hm(d_qkv), stream);
}

extern "C" int mapx_mha_dropout_mask(int64_t B, int F, int H, float p, uint64_t seed, uint64_t offset,
                                     const int32_t* offset_dev_opt, uint8_t* keep, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 0 && F >= 1 && F <= kMhaMaxF && H >= 1 && p >= 0.f && p < 1.f, "mha_dropout_mask: bad arguments");
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(keep, "mha_dropout_mask: null pointer");
  const int64_t rows = B * H * F;
  hipLaunchKernelGGL(mha_mask_kernel, dim3(grid_for(rows * ((F + 3) / 4), 256)), dim3(256), 0, stream, rows, F, p, seed,
                     offset, offset_dev_opt, keep);
  return check_launch("mha_dropout_mask");
}

extern "C" int mapx_field_pool_fwd(const float* x, const float* scores_opt, int64_t B, int F, int E, int mode,
                                   float* out, float* weights_opt, hipStream_t stream) {
  return mapx::field_pool_fwd_launch<float>("field_pool_fwd", x, scores_opt, B, F, E, mode, out, weights_opt, stream);
}

extern "C" int mapx_field_pool_bwd(const float* g, const float* x, const float* weights_opt, int64_t B, int F, int E,
                                   int mode, float* dx, float* d_scores_opt, hipStream_t stream) {
  return mapx::field_pool_bwd_launch<float>("field_pool_bwd", g, x, weights_opt, B, F, E, mode, dx, d_scores_opt,
                                            stream);
}

extern "C" int mapx_field_pool_fwd_bf16(const mapx_bf16* x, const float* scores_opt, int64_t B, int F, int E, int mode,
                                        mapx_bf16* out, float* weights_opt, hipStream_t stream) {
  using namespace mapx;
  return field_pool_fwd_launch<bf16_t>("field_pool_fwd_bf16", hc(x), scores_opt, B, F, E, mode, hm(out), weights_opt,
                                       stream);
}

extern "C" int mapx_field_pool_bwd_bf16(const mapx_bf16* g, const mapx_bf16* x, const float* weights_opt, int64_t B,
                                        int F, int E, int mode, mapx_bf16* dx, float* d_scores_opt,
                                        hipStream_t stream) {
  using namespace mapx;
  return field_pool_bwd_launch<bf16_t>("field_pool_bwd_bf16", hc(g), hc(x), weights_opt, B, F, E, mode, hm(dx),
                                       d_scores_opt, stream);
}
