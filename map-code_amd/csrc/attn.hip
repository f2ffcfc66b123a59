// Self-attention core of the AutoInt backbone (reference code/layers.py:724-744 inside
// MultiHeadAttention.forward :878-909) for field-sized sequences: S = Q K^T (/ sqrt(A)),
// P = softmax(S), O = P V, on G = B*H independent groups of [F, A] (F <= 64 fields, A <= 64).
// The reference splits heads with a plain .view(B*H, -1, A) of the projected [B, F, H*A] tensor, so
// a "group" is simply the g-th run of F*A consecutive floats: no transposes anywhere.
// One wave per group: Q, K, V in LDS, lane i owns query row i.  The problem is tiny (F*F*A MACs)
// and HBM-bound (4 tensors of G*F*A floats); P [G,F,F] is kept for backward.
//
// Dropout forms (attn_drop_*; reference layers.py:740-742 and :901-904, both nn.Dropout(p) of a layer):
//   P~ = P * m_p / (1-p);  O = (P~ V) * m_o / (1-p)      (P is kept undropped)
// Neither keep mask is stored: attn_keep_p / attn_keep_o below are THE definitions, called by forward, backward and
// mapx_attn_dropout_masks.  p = 0 launches the plain kernels.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr int kAttnMaxF = 64, kAttnMaxA = 64;   // one lane per field; LDS budget

// GPW groups per wave: with F <= 32 fields a wave takes TWO groups, one per half (lane & 31 = the query row): the
// one-group form left 41 of 64 lanes idle at Avazu's 23 fields.
template <int GPW>
__global__ void __launch_bounds__(64) attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                      const float* __restrict__ v, int64_t G, int F, int A,
                                                      float inv_scale, float* __restrict__ o, float* __restrict__ p) {
  extern __shared__ float sm[];                 // per group: Q, K, V [F][A+1]; P [F][F+1]
  constexpr int LW = 64 / GPW;                  // lanes per group
  const int LD = A + 1, LF = F + 1;
  const int half = threadIdx.x / LW, li = threadIdx.x % LW;
  float* Qs = sm + half * (3 * F * LD + F * LF);
  float* Ks = Qs + F * LD;
  float* Vs = Ks + F * LD;
  float* Ps = Vs + F * LD;
  const int64_t g = (int64_t)blockIdx.x * GPW + half;
  const bool have = g < G;
  const int64_t base = g * F * A;
  for (int t = li; have && t < F * A; t += LW) {
    const int r = t / A, c = t - r * A;
    Qs[r * LD + c] = q[base + t];
    Ks[r * LD + c] = k[base + t];
    Vs[r * LD + c] = v[base + t];
  }
  __syncthreads();
  const int i = li;
  if (have && i < F) {
    float mx = -3.4e38f;
    for (int j = 0; j < F; ++j) {
      float s = 0.f;
      for (int a = 0; a < A; ++a) s += Qs[i * LD + a] * Ks[j * LD + a];
      s *= inv_scale;
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
    for (int j = 0; j < F; ++j) Ps[i * LF + j] *= rden;
    for (int a = 0; a < A; ++a) {
      float acc = 0.f;
      for (int j = 0; j < F; ++j) acc += Ps[i * LF + j] * Vs[j * LD + a];
      o[base + i * A + a] = acc;
    }
  }
  __syncthreads();
  for (int t = li; have && t < F * F; t += LW) {       // coalesced copy of the probabilities for backward
    const int r = t / F, c = t - r * F;
    p[g * F * F + t] = Ps[r * LF + c];
  }
}

// dV = P^T dO;  dP = dO V^T;  dS = P (dP - rowsum(P dP)) * inv_scale;  dQ = dS K;  dK = dS^T Q
template <int GPW>
__global__ void __launch_bounds__(64) attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                      const float* __restrict__ v, const float* __restrict__ p,
                                                      const float* __restrict__ d_o, int64_t G, int F, int A,
                                                      float inv_scale, float* __restrict__ dq,
                                                      float* __restrict__ dk, float* __restrict__ dv) {
  extern __shared__ float sm[];                 // per group: K, V, Q, dO [F][A+1] each; dS [F][F+1]; P [F][F+1]
  constexpr int LW = 64 / GPW;
  const int LD = A + 1, LF = F + 1;
  const int half = threadIdx.x / LW, li = threadIdx.x % LW;
  float* Ks = sm + half * (4 * F * LD + 2 * F * LF);
  float* Vs = Ks + F * LD;
  float* Qs = Vs + F * LD;
  float* Ds = Qs + F * LD;
  float* dS = Ds + F * LD;
  float* Ps = dS + F * LF;
  const int64_t g = (int64_t)blockIdx.x * GPW + half;
  const bool have = g < G;
  const int64_t base = g * F * A;
  for (int t = li; have && t < F * A; t += LW) {
    const int r = t / A, c = t - r * A;
    Ks[r * LD + c] = k[base + t];
    Vs[r * LD + c] = v[base + t];
    Qs[r * LD + c] = q[base + t];
    Ds[r * LD + c] = d_o[base + t];
  }
  for (int t = li; have && t < F * F; t += LW) {
    const int r = t / F, c = t - r * F;
    Ps[r * LF + c] = p[g * F * F + t];
  }
  __syncthreads();
  const int i = li;
  if (have && i < F) {
    float dot = 0.f;
    for (int j = 0; j < F; ++j) {
      float dp = 0.f;
      for (int a = 0; a < A; ++a) dp += Ds[i * LD + a] * Vs[j * LD + a];
      dS[i * LF + j] = dp;
      dot += Ps[i * LF + j] * dp;
    }
    for (int j = 0; j < F; ++j) dS[i * LF + j] = Ps[i * LF + j] * (dS[i * LF + j] - dot) * inv_scale;
    for (int a = 0; a < A; ++a) {
      float s = 0.f;
      for (int j = 0; j < F; ++j) s += dS[i * LF + j] * Ks[j * LD + a];
      dq[base + i * A + a] = s;
    }
  }
  __syncthreads();
  if (have && i < F) {                           // lane i now owns key / value row i: column sums over queries
    for (int a = 0; a < A; ++a) {
      float sk = 0.f, sv = 0.f;
      for (int r = 0; r < F; ++r) {
        sk += dS[r * LF + i] * Qs[r * LD + a];
        sv += Ps[r * LF + i] * Ds[r * LD + a];
      }
      dk[base + i * A + a] = sk;
      dv[base + i * A + a] = sv;
    }
  }
}

// ---------------------------------------------------------------- dropout forms
__device__ inline uint32_t attn_drop_threshold(float p) { return (uint32_t)fminf(p * 4294967296.0f, 4294967295.0f); }

// What the two masks of one launch are drawn from: Philox(seed, counter, offset + *offset_dev).
struct AttnDrop {
  uint64_t seed, off_p, off_o;
  uint32_t thr;
  int nq4, na4;       // draws per row: ceil(F/4) of the P mask, ceil(A/4) of the O mask
  float rkeep;        // 1 / (1-p)
};

__device__ inline AttnDrop attn_drop_setup(float p, uint64_t seed, uint64_t offset_p, uint64_t offset_o,
                                           const int32_t* offset_dev, int F, int A) {
  const uint64_t add = offset_dev ? (uint64_t)(uint32_t)*offset_dev : 0ull;
  return AttnDrop{seed, offset_p + add, offset_o + add, attn_drop_threshold(p), (F + 3) / 4, (A + 3) / 4,
                  1.f / (1.f - p)};
}

__device__ inline uint32_t attn_keep_bits(const Philox4& r, uint32_t thr) {
  return (uint32_t)(r.x >= thr) | ((uint32_t)(r.y >= thr) << 1) | ((uint32_t)(r.z >= thr) << 2) |
         ((uint32_t)(r.w >= thr) << 3);
}

// P mask: keep bits of keys 4c .. 4c+3 of query row `row` (= g*F + i); bit e set = key 4c+e kept.
__device__ inline uint32_t attn_keep_p(const AttnDrop& d, int64_t row, int c) {
  return attn_keep_bits(philox4x32_10(d.seed, (uint64_t)(row * d.nq4 + c), d.off_p), d.thr);
}

// O mask: keep bits of outputs 4c .. 4c+3 of row `row`; bit e set = output column 4c+e kept.
__device__ inline uint32_t attn_keep_o(const AttnDrop& d, int64_t row, int c) {
  return attn_keep_bits(philox4x32_10(d.seed, (uint64_t)(row * d.na4 + c), d.off_o), d.thr);
}

template <int GPW>
__global__ void __launch_bounds__(64) attn_drop_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, int64_t G, int F, int A,
                                                           float inv_scale, float p, uint64_t seed, uint64_t offset_p,
                                                           uint64_t offset_o, const int32_t* __restrict__ offset_dev,
                                                           float* __restrict__ o, float* __restrict__ probs) {
  extern __shared__ float sm[];                 // per group: Q, K, V [F][A+1]; P (then P~) [F][F+1]
  constexpr int LW = 64 / GPW;
  const int LD = A + 1, LF = F + 1;
  const int half = threadIdx.x / LW, li = threadIdx.x % LW;
  float* Qs = sm + half * (3 * F * LD + F * LF);
  float* Ks = Qs + F * LD;
  float* Vs = Ks + F * LD;
  float* Ps = Vs + F * LD;
  const int64_t g = (int64_t)blockIdx.x * GPW + half;
  const bool have = g < G;
  const int64_t base = g * F * A;
  for (int t = li; have && t < F * A; t += LW) {
    const int r = t / A, c = t - r * A;
    Qs[r * LD + c] = q[base + t];
    Ks[r * LD + c] = k[base + t];
    Vs[r * LD + c] = v[base + t];
  }
  __syncthreads();
  const int i = li;
  if (have && i < F) {
    float mx = -3.4e38f;
    for (int j = 0; j < F; ++j) {
      float s = 0.f;
      for (int a = 0; a < A; ++a) s += Qs[i * LD + a] * Ks[j * LD + a];
      s *= inv_scale;
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
    for (int j = 0; j < F; ++j) Ps[i * LF + j] *= rden;
  }
  __syncthreads();
  for (int t = li; have && t < F * F; t += LW) {       // coalesced copy of the undropped probabilities for backward
    const int r = t / F, c = t - r * F;
    probs[g * F * F + t] = Ps[r * LF + c];
  }
  __syncthreads();
  if (have && i < F) {                                 // row i of P becomes P~ in place, then O = (P~ V) m_o / (1-p)
    const AttnDrop d = attn_drop_setup(p, seed, offset_p, offset_o, offset_dev, F, A);
    const int64_t row = g * F + i;
    uint32_t keep = 0;
    for (int j = 0; j < F; ++j) {
      if ((j & 3) == 0) keep = attn_keep_p(d, row, j >> 2);
      Ps[i * LF + j] = ((keep >> (j & 3)) & 1u) ? Ps[i * LF + j] * d.rkeep : 0.f;
    }
    for (int a = 0; a < A; ++a) {
      if ((a & 3) == 0) keep = attn_keep_o(d, row, a >> 2);
      float acc = 0.f;
      for (int j = 0; j < F; ++j) acc += Ps[i * LF + j] * Vs[j * LD + a];
      o[base + i * A + a] = ((keep >> (a & 3)) & 1u) ? acc * d.rkeep : 0.f;
    }
  }
}

// dO' = dO m_o / (1-p);  dV = P~^T dO';  dP = (dO' V^T) m_p / (1-p);  dS = P (dP - rowsum(P dP)) * inv_scale;
// dQ = dS K;  dK = dS^T Q
template <int GPW>
__global__ void __launch_bounds__(64) attn_drop_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ probs,
                                                           const float* __restrict__ d_o, int64_t G, int F, int A,
                                                           float inv_scale, float p, uint64_t seed, uint64_t offset_p,
                                                           uint64_t offset_o, const int32_t* __restrict__ offset_dev,
                                                           float* __restrict__ dq, float* __restrict__ dk,
                                                           float* __restrict__ dv) {
  extern __shared__ float sm[];                 // per group: K, V, Q, dO' [F][A+1] each; dS [F][F+1]; P, then P~ [F][F+1]
  constexpr int LW = 64 / GPW;
  const int LD = A + 1, LF = F + 1;
  const int half = threadIdx.x / LW, li = threadIdx.x % LW;
  float* Ks = sm + half * (4 * F * LD + 2 * F * LF);
  float* Vs = Ks + F * LD;
  float* Qs = Vs + F * LD;
  float* Ds = Qs + F * LD;
  float* dS = Ds + F * LD;
  float* Ps = dS + F * LF;
  const int64_t g = (int64_t)blockIdx.x * GPW + half;
  const bool have = g < G;
  const int64_t base = g * F * A;
  const AttnDrop d = attn_drop_setup(p, seed, offset_p, offset_o, offset_dev, F, A);
  for (int t = li; have && t < F * A; t += LW) {
    const int r = t / A, c = t - r * A;
    Ks[r * LD + c] = k[base + t];
    Vs[r * LD + c] = v[base + t];
    Qs[r * LD + c] = q[base + t];
  }
  for (int t = li; have && t < F * d.na4; t += LW) {     // dO' staged by the O mask's draws: 4 outputs of a row each
    const int r = t / d.na4, c4 = t - r * d.na4;
    const uint32_t keep = attn_keep_o(d, g * F + r, c4);
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * c4 + e;
      if (c < A) Ds[r * LD + c] = ((keep >> e) & 1u) ? d_o[base + r * A + c] * d.rkeep : 0.f;
    }
  }
  for (int t = li; have && t < F * F; t += LW) {
    const int r = t / F, c = t - r * F;
    Ps[r * LF + c] = probs[g * F * F + t];
  }
  __syncthreads();
  const int i = li;
  if (have && i < F) {
    const int64_t row = g * F + i;
    uint64_t keep = 0;                           // the row's P mask: bit j = key j kept (F <= 64)
    for (int c = 0; c < d.nq4; ++c) keep |= (uint64_t)attn_keep_p(d, row, c) << (4 * c);
    float dot = 0.f;
    for (int j = 0; j < F; ++j) {
      float dp = 0.f;
      for (int a = 0; a < A; ++a) dp += Ds[i * LD + a] * Vs[j * LD + a];
      dp = ((keep >> j) & 1ull) ? dp * d.rkeep : 0.f;
      dS[i * LF + j] = dp;
      dot += Ps[i * LF + j] * dp;
    }
    for (int j = 0; j < F; ++j) {
      const float pij = Ps[i * LF + j];
      dS[i * LF + j] = pij * (dS[i * LF + j] - dot) * inv_scale;
      Ps[i * LF + j] = ((keep >> j) & 1ull) ? pij * d.rkeep : 0.f;      // P~ for dV below
    }
    for (int a = 0; a < A; ++a) {
      float s = 0.f;
      for (int j = 0; j < F; ++j) s += dS[i * LF + j] * Ks[j * LD + a];
      dq[base + i * A + a] = s;
    }
  }
  __syncthreads();
  if (have && i < F) {                           // lane i now owns key / value row i: column sums over queries
    for (int a = 0; a < A; ++a) {
      float sk = 0.f, sv = 0.f;
      for (int r = 0; r < F; ++r) {
        sk += dS[r * LF + i] * Qs[r * LD + a];
        sv += Ps[r * LF + i] * Ds[r * LD + a];
      }
      dk[base + i * A + a] = sk;
      dv[base + i * A + a] = sv;
    }
  }
}

// keep_p [G,F,F], keep_o [G,F,A] (1 = kept): one thread per draw of either mask
__global__ void __launch_bounds__(256) attn_mask_kernel(int64_t rows, int F, int A, float p, uint64_t seed,
                                                        uint64_t offset_p, uint64_t offset_o,
                                                        const int32_t* __restrict__ offset_dev,
                                                        uint8_t* __restrict__ keep_p, uint8_t* __restrict__ keep_o) {
  const AttnDrop d = attn_drop_setup(p, seed, offset_p, offset_o, offset_dev, F, A);
  const int64_t np = rows * d.nq4, n = np + rows * d.na4;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const bool is_p = t < np;
    const int64_t u = is_p ? t : t - np;
    const int n4 = is_p ? d.nq4 : d.na4, W = is_p ? F : A;
    const int64_t row = u / n4;
    const int c = (int)(u - row * n4);
    const uint32_t keep = is_p ? attn_keep_p(d, row, c) : attn_keep_o(d, row, c);
    uint8_t* out = (is_p ? keep_p : keep_o) + row * W;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * c + e < W) out[4 * c + e] = (uint8_t)((keep >> e) & 1u);
  }
}

// F = A = 64 needs 100 KB of dynamic LDS in backward: above the 64 KB default, inside the CU's 160 KB
static hipError_t raise_lds_limit() {
  static hipError_t done = [] {
    for (const void* fn : {reinterpret_cast<const void*>(&attn_fwd_kernel<1>), reinterpret_cast<const void*>(&attn_fwd_kernel<2>),
                           reinterpret_cast<const void*>(&attn_bwd_kernel<1>), reinterpret_cast<const void*>(&attn_bwd_kernel<2>),
                           reinterpret_cast<const void*>(&attn_drop_fwd_kernel<1>), reinterpret_cast<const void*>(&attn_drop_fwd_kernel<2>),
                           reinterpret_cast<const void*>(&attn_drop_bwd_kernel<1>), reinterpret_cast<const void*>(&attn_drop_bwd_kernel<2>)}) {
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }();
  return done;
}

}  // namespace mapx

extern "C" int mapx_attn_fwd(const float* q, const float* k, const float* v, int64_t G, int F, int A, int scaled,
                             float* o, float* p, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(G >= 0 && F >= 1 && F <= kAttnMaxF && A >= 1 && A <= kAttnMaxA,
               "attn_fwd: F <= %d fields, attention size <= %d", kAttnMaxF, kAttnMaxA);
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(q && k && v && o && p, "attn_fwd: null pointer");
  const float inv_scale = scaled ? 1.0f / sqrtf((float)A) : 1.0f;
  const size_t lds = ((size_t)3 * F * (A + 1) + (size_t)F * (F + 1)) * sizeof(float);
  MAPX_HIP(raise_lds_limit());
  if (F <= 32)
    hipLaunchKernelGGL(attn_fwd_kernel<2>, dim3((unsigned)((G + 1) / 2)), dim3(64), 2 * lds, stream, q, k, v, G, F, A,
                       inv_scale, o, p);
  else
    hipLaunchKernelGGL(attn_fwd_kernel<1>, dim3((unsigned)G), dim3(64), lds, stream, q, k, v, G, F, A, inv_scale, o, p);
  return check_launch("attn_fwd");
}

extern "C" int mapx_attn_bwd(const float* q, const float* k, const float* v, const float* p, const float* d_o,
                             int64_t G, int F, int A, int scaled, float* dq, float* dk, float* dv,
                             hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(G >= 0 && F >= 1 && F <= kAttnMaxF && A >= 1 && A <= kAttnMaxA,
               "attn_bwd: F <= %d fields, attention size <= %d", kAttnMaxF, kAttnMaxA);
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(q && k && v && p && d_o && dq && dk && dv, "attn_bwd: null pointer");
  const float inv_scale = scaled ? 1.0f / sqrtf((float)A) : 1.0f;
  const size_t lds = ((size_t)4 * F * (A + 1) + (size_t)2 * F * (F + 1)) * sizeof(float);
  MAPX_HIP(raise_lds_limit());
  if (F <= 32)
    hipLaunchKernelGGL(attn_bwd_kernel<2>, dim3((unsigned)((G + 1) / 2)), dim3(64), 2 * lds, stream, q, k, v, p, d_o, G,
                       F, A, inv_scale, dq, dk, dv);
  else
    hipLaunchKernelGGL(attn_bwd_kernel<1>, dim3((unsigned)G), dim3(64), lds, stream, q, k, v, p, d_o, G, F, A,
                       inv_scale, dq, dk, dv);
  return check_launch("attn_bwd");
}

static int attn_drop_check(const char* what, int64_t G, int F, int A, float p) {
  using namespace mapx;
  MAPX_REQUIRE(G >= 0 && F >= 1 && F <= kAttnMaxF && A >= 1 && A <= kAttnMaxA && p >= 0.f && p < 1.f,
               "%s: F <= %d fields, attention size <= %d, 0 <= p < 1 (got F=%d A=%d p=%g)", what, kAttnMaxF, kAttnMaxA, F,
               A, (double)p);
  return MAPX_OK;
}

extern "C" int mapx_attn_drop_fwd(const float* q, const float* k, const float* v, int64_t G, int F, int A, int scaled,
                                  float p, uint64_t seed, uint64_t offset_p, uint64_t offset_o,
                                  const int32_t* offset_dev_opt, float* o, float* probs, hipStream_t stream) {
  using namespace mapx;
  if (int st = attn_drop_check("attn_drop_fwd", G, F, A, p)) return st;
  if (p == 0.f) return mapx_attn_fwd(q, k, v, G, F, A, scaled, o, probs, stream);
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(q && k && v && o && probs, "attn_drop_fwd: null pointer");
  const float inv_scale = scaled ? 1.0f / sqrtf((float)A) : 1.0f;
  const size_t lds = ((size_t)3 * F * (A + 1) + (size_t)F * (F + 1)) * sizeof(float);
  MAPX_HIP(raise_lds_limit());
  if (F <= 32)
    hipLaunchKernelGGL(attn_drop_fwd_kernel<2>, dim3((unsigned)((G + 1) / 2)), dim3(64), 2 * lds, stream, q, k, v, G, F, A,
                       inv_scale, p, seed, offset_p, offset_o, offset_dev_opt, o, probs);
  else
    hipLaunchKernelGGL(attn_drop_fwd_kernel<1>, dim3((unsigned)G), dim3(64), lds, stream, q, k, v, G, F, A, inv_scale, p,
                       seed, offset_p, offset_o, offset_dev_opt, o, probs);
  return check_launch("attn_drop_fwd");
}

extern "C" int mapx_attn_drop_bwd(const float* q, const float* k, const float* v, const float* probs, const float* d_o,
                                  int64_t G, int F, int A, int scaled, float p, uint64_t seed, uint64_t offset_p,
                                  uint64_t offset_o, const int32_t* offset_dev_opt, float* dq, float* dk, float* dv,
                                  hipStream_t stream) {
  using namespace mapx;
  if (int st = attn_drop_check("attn_drop_bwd", G, F, A, p)) return st;
  if (p == 0.f) return mapx_attn_bwd(q, k, v, probs, d_o, G, F, A, scaled, dq, dk, dv, stream);
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(q && k && v && probs && d_o && dq && dk && dv, "attn_drop_bwd: null pointer");
  const float inv_scale = scaled ? 1.0f / sqrtf((float)A) : 1.0f;
  const size_t lds = ((size_t)4 * F * (A + 1) + (size_t)2 * F * (F + 1)) * sizeof(float);
  MAPX_HIP(raise_lds_limit());
  if (F <= 32)
    hipLaunchKernelGGL(attn_drop_bwd_kernel<2>, dim3((unsigned)((G + 1) / 2)), dim3(64), 2 * lds, stream, q, k, v, probs,
                       d_o, G, F, A, inv_scale, p, seed, offset_p, offset_o, offset_dev_opt, dq, dk, dv);
  else
    hipLaunchKernelGGL(attn_drop_bwd_kernel<1>, dim3((unsigned)G), dim3(64), lds, stream, q, k, v, probs, d_o, G, F, A,
                       inv_scale, p, seed, offset_p, offset_o, offset_dev_opt, dq, dk, dv);
  return check_launch("attn_drop_bwd");
}

extern "C" int mapx_attn_dropout_masks(int64_t G, int F, int A, float p, uint64_t seed, uint64_t offset_p,
                                       uint64_t offset_o, const int32_t* offset_dev_opt, uint8_t* keep_p,
                                       uint8_t* keep_o, hipStream_t stream) {
  using namespace mapx;
  if (int st = attn_drop_check("attn_dropout_masks", G, F, A, p)) return st;
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(keep_p && keep_o, "attn_dropout_masks: null pointer");
  const int64_t rows = G * F;
  hipLaunchKernelGGL(attn_mask_kernel, dim3(grid_for(rows * ((F + 3) / 4 + (A + 3) / 4), 256)), dim3(256), 0, stream, rows,
                     F, A, p, seed, offset_p, offset_o, offset_dev_opt, keep_p, keep_o);
  return check_launch("attn_dropout_masks");
}
