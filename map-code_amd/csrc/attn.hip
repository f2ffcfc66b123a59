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
// Neither keep mask is stored: forward, backward and mapx_attn_dropout_masks regenerate them through attn_keep_p /
// attn_keep_o below, which give the one dropout draw (common.h: drop_threshold, drop_offset, keep_bits4) their counters.
// One forward and one backward kernel template; DROP = false (p = 0) is the plain form.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr int kAttnMaxF = 64, kAttnMaxA = 64;   // one lane per field; LDS budget

// Element type T of q, k, v, o, dO, dq, dk, dv: float, or bf16_t (bf16 compute mode).  Only the global
// loads and stores differ: a load widens to fp32 into the LDS staging (which stays fp32: the same LDS budget), all
// arithmetic is the fp32 code below, a store rounds to nearest even once.  P is fp32 for both.  (bf16_t and its
// vector types: common.h.)

// Elements per staging load.  A group starts at element g*F*A, which is only 2-byte aligned when F*A is odd: 8-byte
// loads when F*A % 4 == 0, 4-byte ones when it is even, single elements otherwise (A = 7, A = 1 with odd F).
template <class T>
__device__ inline int attn_vec(int FA, const void* a, const void* b, const void* c, const void* d) {
  if constexpr (sizeof(T) == 4) {
    return 1;
  } else {
    const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d;
    return (FA % 4 == 0 && bits % 8 == 0) ? 4 : ((FA % 2 == 0 && bits % 4 == 0) ? 2 : 1);
  }
}

template <int V, class T>
__device__ inline void attn_load(const T* __restrict__ p, float (&f)[V]) {
  if constexpr (V == 4) {
    const float4 v = load4(p);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else if constexpr (V == 2) {
    const bf16x2_t v = *reinterpret_cast<const bf16x2_t*>(p);
    f[0] = (float)v[0]; f[1] = (float)v[1];
  } else {
    f[0] = (float)p[0];
  }
}

// Stages NT tensors' [F*A] elements of one group into their padded LDS rows [F][LD], V elements per load.
template <int V, int NT, class T>
__device__ inline void attn_stage_v(const T* const (&src)[NT], float* const (&dst)[NT], int64_t base, int FA, int A,
                                    int LD, int li, int LW) {
  for (int t = V * li; t < FA; t += V * LW) {
    float f[NT][V];
#pragma unroll
    for (int n = 0; n < NT; ++n) attn_load<V>(src[n] + base + t, f[n]);
    int r = t / A, c = t - r * A;
#pragma unroll
    for (int e = 0; e < V; ++e) {
#pragma unroll
      for (int n = 0; n < NT; ++n) dst[n][r * LD + c] = f[n][e];
      if (++c == A) { c = 0; ++r; }
    }
  }
}

template <int NT, class T>
__device__ inline void attn_stage(const T* const (&src)[NT], float* const (&dst)[NT], int64_t base, int FA, int A,
                                  int LD, int li, int LW, int vec) {
  if constexpr (sizeof(T) == 4) {
    attn_stage_v<1>(src, dst, base, FA, A, LD, li, LW);
  } else {
    if (vec == 4) attn_stage_v<4>(src, dst, base, FA, A, LD, li, LW);
    else if (vec == 2) attn_stage_v<2>(src, dst, base, FA, A, LD, li, LW);
    else attn_stage_v<1>(src, dst, base, FA, A, LD, li, LW);
  }
}

// One lane's output row [A]: put(a, v) for a = 0 .. A-1 in order.  bf16 with an even A on 4-byte aligned rows: the
// even column waits in a register for the odd one and both leave as one 4-byte store.
template <class T>
struct AttnRowOut {
  T* p;
  bool pair;
  float held;
  __device__ inline AttnRowOut(T* row, int A) : p(row), pair(sizeof(T) == 2 && A % 2 == 0 && (uintptr_t)row % 4 == 0), held(0.f) {}
  __device__ inline void put(int a, float v) {
    if constexpr (sizeof(T) == 4) {
      p[a] = v;
    } else {
      if (!pair) {
        p[a] = (T)v;                                   // v_cvt_pk_bf16_f32: round to nearest even
      } else if (a & 1) {
        bf16x2_t o;
        o[0] = (bf16_t)held; o[1] = (bf16_t)v;
        *reinterpret_cast<bf16x2_t*>(p + a - 1) = o;
      } else {
        held = v;
      }
    }
  }
};

// ---------------------------------------------------------------- dropout
// What a dropout launch is given: the kernels' last parameter when DROP, a parameter the plain kernels do not have
// (`DA... da` below is AttnDropArgs or nothing), so the plain kernel-argument block carries none of this.
struct AttnDropArgs {
  float p;
  uint64_t seed, offset_p, offset_o;
  const int32_t* offset_dev;
};

// What the two masks of one launch are drawn from: Philox(seed, counter, offset + *offset_dev) (common.h).
struct AttnDrop {
  uint64_t seed, off_p, off_o;
  uint32_t thr;
  int nq4, na4;       // draws per row: ceil(F/4) of the P mask, ceil(A/4) of the O mask
  float rkeep;        // 1 / (1-p)
};

__device__ inline AttnDrop attn_drop_setup(const AttnDropArgs& a, int F, int A) {
  return AttnDrop{a.seed, drop_offset(a.offset_p, a.offset_dev), drop_offset(a.offset_o, a.offset_dev),
                  drop_threshold(a.p), (F + 3) / 4, (A + 3) / 4, 1.f / (1.f - a.p)};
}

// P mask: keep bits of keys 4c .. 4c+3 of query row `row` (= g*F + i); bit e set = key 4c+e kept.
__device__ inline uint32_t attn_keep_p(const AttnDrop& d, int64_t row, int c) {
  return keep_bits4(philox4x32_10(d.seed, (uint64_t)(row * d.nq4 + c), d.off_p), d.thr);
}

// O mask: keep bits of outputs 4c .. 4c+3 of row `row`; bit e set = output column 4c+e kept.
__device__ inline uint32_t attn_keep_o(const AttnDrop& d, int64_t row, int c) {
  return keep_bits4(philox4x32_10(d.seed, (uint64_t)(row * d.na4 + c), d.off_o), d.thr);
}

// ---------------------------------------------------------------- kernels
// GPW groups per wave: with F <= 32 fields a wave takes TWO groups, one per half (lane & 31 = the query row): the
// one-group form left 41 of 64 lanes idle at Avazu's 23 fields.
// DROP = false: O is formed in the softmax block, then P is copied out.  DROP = true: the undropped P is copied out
// first, then row i of P becomes P~ in place and O = (P~ V) m_o / (1-p).
template <int GPW, bool DROP, class T, class... DA>
__global__ void __launch_bounds__(64) attn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                      const T* __restrict__ v, int64_t G, int F, int A,
                                                      float inv_scale, T* __restrict__ o, float* __restrict__ p,
                                                      DA... da) {
  static_assert(sizeof...(DA) == (DROP ? 1 : 0), "AttnDropArgs exactly when DROP");
  extern __shared__ float sm[];                 // per group: Q, K, V [F][A+1]; P (DROP: then P~) [F][F+1]
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
  if (have) {
    const T* const src[3] = {q, k, v};
    float* const dst[3] = {Qs, Ks, Vs};
    attn_stage(src, dst, base, F * A, A, LD, li, LW, attn_vec<T>(F * A, q, k, v, nullptr));
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
    if constexpr (!DROP) {
      AttnRowOut<T> orow(o + base + i * A, A);
      for (int a = 0; a < A; ++a) {
        float acc = 0.f;
        for (int j = 0; j < F; ++j) acc += Ps[i * LF + j] * Vs[j * LD + a];
        orow.put(a, acc);
      }
    }
  }
  __syncthreads();
  for (int t = li; have && t < F * F; t += LW) {       // coalesced copy of the (undropped) probabilities for backward
    const int r = t / F, c = t - r * F;
    p[g * F * F + t] = Ps[r * LF + c];
  }
  if constexpr (DROP) {
    __syncthreads();
    if (have && i < F) {
      const AttnDrop d = attn_drop_setup(da..., F, A);
      const int64_t row = g * F + i;
      uint32_t keep = 0;
      for (int j = 0; j < F; ++j) {
        if ((j & 3) == 0) keep = attn_keep_p(d, row, j >> 2);
        Ps[i * LF + j] = ((keep >> (j & 3)) & 1u) ? Ps[i * LF + j] * d.rkeep : 0.f;
      }
      AttnRowOut<T> orow(o + base + i * A, A);
      for (int a = 0; a < A; ++a) {
        if ((a & 3) == 0) keep = attn_keep_o(d, row, a >> 2);
        float acc = 0.f;
        for (int j = 0; j < F; ++j) acc += Ps[i * LF + j] * Vs[j * LD + a];
        orow.put(a, ((keep >> (a & 3)) & 1u) ? acc * d.rkeep : 0.f);
      }
    }
  }
}

// dV = P^T dO;  dP = dO V^T;  dS = P (dP - rowsum(P dP)) * inv_scale;  dQ = dS K;  dK = dS^T Q
// DROP: dO' = dO m_o / (1-p) in place of dO, P~ in place of P in dV, and dP = (dO' V^T) m_p / (1-p).
template <int GPW, bool DROP, class T, class... DA>
__global__ void __launch_bounds__(64) attn_bwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                      const T* __restrict__ v, const float* __restrict__ p,
                                                      const T* __restrict__ d_o, int64_t G, int F, int A,
                                                      float inv_scale, T* __restrict__ dq, T* __restrict__ dk,
                                                      T* __restrict__ dv, DA... da) {
  static_assert(sizeof...(DA) == (DROP ? 1 : 0), "AttnDropArgs exactly when DROP");
  extern __shared__ float sm[];    // per group: K, V, Q, dO (dO') [F][A+1] each; dS [F][F+1]; P (DROP: then P~) [F][F+1]
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
  AttnDrop d;
  if constexpr (DROP) {
    d = attn_drop_setup(da..., F, A);
    if (have) {
      const T* const src[3] = {k, v, q};
      float* const dst[3] = {Ks, Vs, Qs};
      attn_stage(src, dst, base, F * A, A, LD, li, LW, attn_vec<T>(F * A, q, k, v, nullptr));
    }
    for (int t = li; have && t < F * d.na4; t += LW) {   // dO' staged by the O mask's draws: 4 outputs of a row each
      const int r = t / d.na4, c4 = t - r * d.na4;
      const uint32_t keep = attn_keep_o(d, g * F + r, c4);
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * c4 + e;
        if (c < A) Ds[r * LD + c] = ((keep >> e) & 1u) ? (float)d_o[base + r * A + c] * d.rkeep : 0.f;
      }
    }
  } else if (have) {
    const T* const src[4] = {k, v, q, d_o};
    float* const dst[4] = {Ks, Vs, Qs, Ds};
    attn_stage(src, dst, base, F * A, A, LD, li, LW, attn_vec<T>(F * A, q, k, v, d_o));
  }
  for (int t = li; have && t < F * F; t += LW) {
    const int r = t / F, c = t - r * F;
    Ps[r * LF + c] = p[g * F * F + t];
  }
  __syncthreads();
  const int i = li;
  if (have && i < F) {
    uint64_t keep = 0;                           // DROP: the row's P mask, bit j = key j kept (F <= 64)
    if constexpr (DROP)
      for (int c = 0; c < d.nq4; ++c) keep |= (uint64_t)attn_keep_p(d, g * F + i, c) << (4 * c);
    float dot = 0.f;
    for (int j = 0; j < F; ++j) {
      float dp = 0.f;
      for (int a = 0; a < A; ++a) dp += Ds[i * LD + a] * Vs[j * LD + a];
      if constexpr (DROP) dp = ((keep >> j) & 1ull) ? dp * d.rkeep : 0.f;
      dS[i * LF + j] = dp;
      dot += Ps[i * LF + j] * dp;
    }
    for (int j = 0; j < F; ++j) {
      const float pij = Ps[i * LF + j];
      dS[i * LF + j] = pij * (dS[i * LF + j] - dot) * inv_scale;
      if constexpr (DROP) Ps[i * LF + j] = ((keep >> j) & 1ull) ? pij * d.rkeep : 0.f;      // P~ for dV below
    }
    AttnRowOut<T> qrow(dq + base + i * A, A);
    for (int a = 0; a < A; ++a) {
      float s = 0.f;
      for (int j = 0; j < F; ++j) s += dS[i * LF + j] * Ks[j * LD + a];
      qrow.put(a, s);
    }
  }
  __syncthreads();
  if (have && i < F) {                           // lane i now owns key / value row i: column sums over queries
    AttnRowOut<T> krow(dk + base + i * A, A), vrow(dv + base + i * A, A);
    for (int a = 0; a < A; ++a) {
      float sk = 0.f, sv = 0.f;
      for (int r = 0; r < F; ++r) {
        sk += dS[r * LF + i] * Qs[r * LD + a];
        sv += Ps[r * LF + i] * Ds[r * LD + a];
      }
      krow.put(a, sk);
      vrow.put(a, sv);
    }
  }
}

// keep_p [G,F,F], keep_o [G,F,A] (1 = kept): one thread per draw of either mask
__global__ void __launch_bounds__(256) attn_mask_kernel(int64_t rows, int F, int A, AttnDropArgs da,
                                                        uint8_t* __restrict__ keep_p, uint8_t* __restrict__ keep_o) {
  const AttnDrop d = attn_drop_setup(da, F, A);
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

// ---------------------------------------------------------------- host
static int attn_drop_check(const char* what, int64_t G, int F, int A, float p) {
  MAPX_REQUIRE(G >= 0 && F >= 1 && F <= kAttnMaxF && A >= 1 && A <= kAttnMaxA && p >= 0.f && p < 1.f,
               "%s: F <= %d fields, attention size <= %d, 0 <= p < 1 (got F=%d A=%d p=%g)", what, kAttnMaxF, kAttnMaxA, F,
               A, (double)p);
  return MAPX_OK;
}

// What every launch starts with.  A dropout entry names the plain entry it becomes at p = 0 (`plain`; null for a
// plain entry): from there on it reports under that name.  nbuf [F][A+1] and npr [F][F+1] fp32 LDS arrays per group.
static int attn_prepare(const char*& what, const char* plain, int64_t G, int F, int A, int scaled, float p, int nbuf,
                        int npr, float& inv_scale, size_t& lds) {
  if (plain) {
    if (int st = attn_drop_check(what, G, F, A, p)) return st;
    if (p == 0.f) what = plain;
  }
  MAPX_REQUIRE(G >= 0 && F >= 1 && F <= kAttnMaxF && A >= 1 && A <= kAttnMaxA,
               "%s: F <= %d fields, attention size <= %d", what, kAttnMaxF, kAttnMaxA);
  inv_scale = scaled ? 1.0f / sqrtf((float)A) : 1.0f;
  lds = ((size_t)nbuf * F * (A + 1) + (size_t)npr * F * (F + 1)) * sizeof(float);
  return MAPX_OK;
}

// F = A = 64 needs 100 KB of dynamic LDS in backward: above the 64 KB default, inside the CU's 160 KB
template <class T>
static hipError_t attn_allow_lds() {
  static const hipError_t done = allow_dynamic_lds(
      128 * 1024, &attn_fwd_kernel<1, false, T>, &attn_fwd_kernel<2, false, T>,
      &attn_fwd_kernel<1, true, T, AttnDropArgs>, &attn_fwd_kernel<2, true, T, AttnDropArgs>,
      &attn_bwd_kernel<1, false, T>, &attn_bwd_kernel<2, false, T>, &attn_bwd_kernel<1, true, T, AttnDropArgs>,
      &attn_bwd_kernel<2, true, T, AttnDropArgs>);
  return done;
}

// GPW = 2 when F <= 32; DROP = false, without the dropout arguments, when p == 0
#define MAPX_ATTN_LAUNCH(KERNEL, ...)                                                                                \
  do {                                                                                                               \
    const dim3 grid((unsigned)(F <= 32 ? (G + 1) / 2 : G));                                                          \
    if (F <= 32 && da.p == 0.f)                                                                                      \
      hipLaunchKernelGGL((KERNEL<2, false, T>), grid, dim3(64), 2 * lds, stream, __VA_ARGS__);                       \
    else if (da.p == 0.f)                                                                                            \
      hipLaunchKernelGGL((KERNEL<1, false, T>), grid, dim3(64), lds, stream, __VA_ARGS__);                           \
    else if (F <= 32)                                                                                                \
      hipLaunchKernelGGL((KERNEL<2, true, T, AttnDropArgs>), grid, dim3(64), 2 * lds, stream, __VA_ARGS__, da);      \
    else                                                                                                             \
      hipLaunchKernelGGL((KERNEL<1, true, T, AttnDropArgs>), grid, dim3(64), lds, stream, __VA_ARGS__, da);          \
  } while (0)

template <class T>
static int attn_fwd_launch(const char* what, const char* plain, const T* q, const T* k, const T* v, int64_t G, int F,
                           int A, int scaled, const AttnDropArgs& da, T* o, float* p, hipStream_t stream) {
  float inv_scale;
  size_t lds;
  if (int st = attn_prepare(what, plain, G, F, A, scaled, da.p, 3, 1, inv_scale, lds)) return st;
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(q && k && v && o && p, "%s: null pointer", what);
  MAPX_HIP(attn_allow_lds<T>());
  MAPX_ATTN_LAUNCH(attn_fwd_kernel, q, k, v, G, F, A, inv_scale, o, p);
  return check_launch(what);
}

template <class T>
static int attn_bwd_launch(const char* what, const char* plain, const T* q, const T* k, const T* v, const float* p,
                           const T* d_o, int64_t G, int F, int A, int scaled, const AttnDropArgs& da, T* dq, T* dk,
                           T* dv, hipStream_t stream) {
  float inv_scale;
  size_t lds;
  if (int st = attn_prepare(what, plain, G, F, A, scaled, da.p, 4, 2, inv_scale, lds)) return st;
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(q && k && v && p && d_o && dq && dk && dv, "%s: null pointer", what);
  MAPX_HIP(attn_allow_lds<T>());
  MAPX_ATTN_LAUNCH(attn_bwd_kernel, q, k, v, p, d_o, G, F, A, inv_scale, dq, dk, dv);
  return check_launch(what);
}
#undef MAPX_ATTN_LAUNCH

static const AttnDropArgs kNoDrop = {0.f, 0, 0, 0, nullptr};

}  // namespace mapx

extern "C" int mapx_attn_fwd(const float* q, const float* k, const float* v, int64_t G, int F, int A, int scaled,
                             float* o, float* p, hipStream_t stream) {
  using namespace mapx;
  return attn_fwd_launch<float>("attn_fwd", nullptr, q, k, v, G, F, A, scaled, kNoDrop, o, p, stream);
}

extern "C" int mapx_attn_bwd(const float* q, const float* k, const float* v, const float* p, const float* d_o,
                             int64_t G, int F, int A, int scaled, float* dq, float* dk, float* dv,
                             hipStream_t stream) {
  using namespace mapx;
  return attn_bwd_launch<float>("attn_bwd", nullptr, q, k, v, p, d_o, G, F, A, scaled, kNoDrop, dq, dk, dv, stream);
}

extern "C" int mapx_attn_drop_fwd(const float* q, const float* k, const float* v, int64_t G, int F, int A, int scaled,
                                  float p, uint64_t seed, uint64_t offset_p, uint64_t offset_o,
                                  const int32_t* offset_dev_opt, float* o, float* probs, hipStream_t stream) {
  using namespace mapx;
  return attn_fwd_launch<float>("attn_drop_fwd", "attn_fwd", q, k, v, G, F, A, scaled,
                                {p, seed, offset_p, offset_o, offset_dev_opt}, o, probs, stream);
}

extern "C" int mapx_attn_drop_bwd(const float* q, const float* k, const float* v, const float* probs, const float* d_o,
                                  int64_t G, int F, int A, int scaled, float p, uint64_t seed, uint64_t offset_p,
                                  uint64_t offset_o, const int32_t* offset_dev_opt, float* dq, float* dk, float* dv,
                                  hipStream_t stream) {
  using namespace mapx;
  return attn_bwd_launch<float>("attn_drop_bwd", "attn_bwd", q, k, v, probs, d_o, G, F, A, scaled,
                                {p, seed, offset_p, offset_o, offset_dev_opt}, dq, dk, dv, stream);
}

// bf16 I/O forms: the same kernel templates on bf16 elements (q, k, v, dO in; o, dq, dk, dv out); P stays fp32.
extern "C" int mapx_attn_fwd_bf16(const mapx_bf16* q, const mapx_bf16* k, const mapx_bf16* v, int64_t G, int F, int A,
                                  int scaled, mapx_bf16* o, float* p, hipStream_t stream) {
  using namespace mapx;
  return attn_fwd_launch<bf16_t>("attn_fwd_bf16", nullptr, hc(q), hc(k), hc(v), G, F, A, scaled, kNoDrop, hm(o), p,
                                 stream);
}

extern "C" int mapx_attn_bwd_bf16(const mapx_bf16* q, const mapx_bf16* k, const mapx_bf16* v, const float* p,
                                  const mapx_bf16* d_o, int64_t G, int F, int A, int scaled, mapx_bf16* dq,
                                  mapx_bf16* dk, mapx_bf16* dv, hipStream_t stream) {
  using namespace mapx;
  return attn_bwd_launch<bf16_t>("attn_bwd_bf16", nullptr, hc(q), hc(k), hc(v), p, hc(d_o), G, F, A, scaled, kNoDrop,
                                 hm(dq), hm(dk), hm(dv), stream);
}

extern "C" int mapx_attn_drop_fwd_bf16(const mapx_bf16* q, const mapx_bf16* k, const mapx_bf16* v, int64_t G, int F,
                                       int A, int scaled, float p, uint64_t seed, uint64_t offset_p, uint64_t offset_o,
                                       const int32_t* offset_dev_opt, mapx_bf16* o, float* probs, hipStream_t stream) {
  using namespace mapx;
  return attn_fwd_launch<bf16_t>("attn_drop_fwd_bf16", "attn_fwd_bf16", hc(q), hc(k), hc(v), G, F, A, scaled,
                                 {p, seed, offset_p, offset_o, offset_dev_opt}, hm(o), probs, stream);
}

extern "C" int mapx_attn_drop_bwd_bf16(const mapx_bf16* q, const mapx_bf16* k, const mapx_bf16* v, const float* probs,
                                       const mapx_bf16* d_o, int64_t G, int F, int A, int scaled, float p, uint64_t seed,
                                       uint64_t offset_p, uint64_t offset_o, const int32_t* offset_dev_opt, mapx_bf16* dq,
                                       mapx_bf16* dk, mapx_bf16* dv, hipStream_t stream) {
  using namespace mapx;
  return attn_bwd_launch<bf16_t>("attn_drop_bwd_bf16", "attn_bwd_bf16", hc(q), hc(k), hc(v), probs, hc(d_o), G, F, A,
                                 scaled, {p, seed, offset_p, offset_o, offset_dev_opt}, hm(dq), hm(dk), hm(dv), stream);
}

extern "C" int mapx_attn_dropout_masks(int64_t G, int F, int A, float p, uint64_t seed, uint64_t offset_p,
                                       uint64_t offset_o, const int32_t* offset_dev_opt, uint8_t* keep_p,
                                       uint8_t* keep_o, hipStream_t stream) {
  using namespace mapx;
  if (int st = mapx::attn_drop_check("attn_dropout_masks", G, F, A, p)) return st;
  if (G == 0) return MAPX_OK;
  MAPX_REQUIRE(keep_p && keep_o, "attn_dropout_masks: null pointer");
  const int64_t rows = G * F;
  hipLaunchKernelGGL(attn_mask_kernel, dim3(grid_for(rows * ((F + 3) / 4 + (A + 3) / 4), 256)), dim3(256), 0, stream, rows,
                     F, A, AttnDropArgs{p, seed, offset_p, offset_o, offset_dev_opt}, keep_p, keep_o);
  return check_launch("attn_dropout_masks");
}
