// Compressed Interaction Network in bf16 compute mode (xDeepFM; reference code/layers.py:696-721) without the Hadamard
// matrix.  Rows r = (b, d), R = B*E, activations embedding-major as in cin.hip.  One layer is
//   Y[r, o] = bias[o] + sum_{h < F, m < H} W[o, h*H + m] * a[r, h*H + m],   a[r, h*H + m] = bf16(x0t[r, h] * xi[r, m])
// (the product of two bf16 values is exact in fp32; it is rounded once, where it becomes the MFMA operand).  cin.hip
// writes a as an R x F*H matrix (302 MB in fp32 at Avazu's sizes, read by three GEMMs, plus its gradient); here a and
// its gradient dA = dY W exist only as MFMA fragments / accumulators of v_mfma_f32_32x32x16_bf16.
//
// All three kernels walk the fields h one at a time, so the split k -> (h, m) is two loop counters and no division:
// the weight's slice W[:, h*H .. h*H + H) goes to LDS (zero-filled to the tile, which also takes care of an odd
// F*H: the shadow is read with 2-byte loads, coalesced along k), x0t[r, h] is one scalar per row and the row's xi
// sits in registers at STATIC indices that match the MFMA layout:
//   forward   A = a (rows r, 8 consecutive m per lane = the row's xi registers times x0t[r, h]), B = W slice.
//   dX        C^T[m][r] = sum_o W[o, hH + m] dY[r, o]: the lane owns ONE row r and 16 values of m per tile, so
//             dxi[r, m] += dA x0t[r, h] is a register FMA and dx0t[r, h] = sum_m dA xi[r, m] a lane-local sum plus one
//             exchange between the wave's halves (fixed order, no atomics).
//   dW        rows of a slab are staged transposed in LDS; a wave owns one field h and 32 output units and recomputes
//             a[r, (h, m)] from the two transposed tiles; fp32 slab partials are added in slab order.
// fp32 accumulation everywhere, 0 bytes of scratch (DESIGN §4.6 has the compiler's register report).
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kCinMaxF = 64;       // fields (also layer 1's H)
constexpr int kCinMaxH = 128;      // units of a layer = the next layer's H
constexpr int kCinRows = 128;      // rows per workgroup of the forward / dX kernels: 4 waves x 32
constexpr int kDwChunk = 64;       // rows per LDS stage of the dW kernel (4 MFMA k-steps)
constexpr int kDwPitch = kDwChunk + 8;
constexpr int kDwSlabRows = 256;   // a slab is at least this many rows ...
constexpr int kDwMaxSlabs = 64;    // ... and there are at most this many

__device__ inline bf16_t bzero() { return (bf16_t)0.f; }

// C/D layout of v_mfma_f32_32x32x16_bf16: column = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5).
__device__ inline int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// x0s[rr * pF + f] = x0t[row0 + rr, f] for the workgroup's 128 rows (zeros behind R)
__device__ inline void stage_x0(const bf16_t* __restrict__ x0t, int ld0, int F, int64_t row0, int64_t R,
                                bf16_t* __restrict__ x0s, int pF) {
  const int col = threadIdx.x & 63;
  if (col < F)
    for (int rr = threadIdx.x >> 6; rr < kCinRows; rr += 4)
      x0s[rr * pF + col] = row0 + rr < R ? x0t[(row0 + rr) * ld0 + col] : bzero();
}

// ---------------------------------------------------------------- forward
template <int NTU>
__global__ void __launch_bounds__(256) cin_fused_fwd_kernel(const bf16_t* __restrict__ x0t, int ld0, int F,
                                                            const bf16_t* __restrict__ xi, int ldi, int H,
                                                            const bf16_t* __restrict__ W,
                                                            const float* __restrict__ bias, int U, int64_t R,
                                                            bf16_t* __restrict__ Y, int ldy) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int Hp = (H + 15) & ~15, pw = Hp + 8, pF = F | 1, K = F * H;
  bf16_t* __restrict__ Ws = reinterpret_cast<bf16_t*>(smem);         // [NTU * 32][pw]: W[o, h*H + m], zero-filled
  bf16_t* __restrict__ x0s = Ws + NTU * 32 * pw;                     // [128][pF]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, hh = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * kCinRows, row = row0 + wave * 32 + lr;
  const bool valid = row < R;
  stage_x0(x0t, ld0, F, row0, R, x0s, pF);
  // the row's xi in the A operand's order: k-step s holds m = 16 s + 8 hh + j
  float xr[kCinMaxH / 16][8];
#pragma unroll
  for (int s = 0; s < kCinMaxH / 16; ++s) {
    const int m0 = 16 * s + 8 * hh;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (valid && m0 < ldi && 16 * s < H) {
      lo = load4(xi + row * ldi + m0);
      hi = load4(xi + row * ldi + m0 + 4);
    }
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) xr[s][j] = m0 + j < H ? v[j] : 0.f;
  }
  f32x16 acc[NTU];
#pragma unroll
  for (int t = 0; t < NTU; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  // The slice as 256 threads copy it: its columns rounded up to a power of two, thread tid takes column tid % MW of rows
  // tid / MW + i * (256 / MW); coalesced 2-byte loads of the shadow (F*H may be odd), a uniform stride between a
  // thread's elements.  All loads are issued before the barrier behind which the previous slice is free, and land in
  // LDS after it.  (One load, one store at a time, 32 times per field, was the kernel's whole time: 154 us per layer.
  // Holding slice h + 1 in registers across the MFMAs of slice h doubled the VGPRs and put the four-tile dX kernel into
  // scratch.)
  constexpr int NW = NTU * 16;                              // rows per thread at MW = 128
  const int lg = Hp <= 16 ? 4 : Hp <= 32 ? 5 : Hp <= 64 ? 6 : 7;
  const int wm = tid & ((1 << lg) - 1), wo = tid >> lg, wstep = 256 >> lg;
  bf16_t wv[NW];
  for (int h = 0; h < F; ++h) {
    const int base = h * H + wm;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int o = wo + i * wstep;
      wv[i] = (o < U && wm < H) ? W[o * K + base] : bzero();          // (U * K <= 2^19)
    }
    __syncthreads();                                        // the previous slice has been consumed
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int o = wo + i * wstep;
      if (o < NTU * 32 && wm < Hp) Ws[o * pw + wm] = wv[i];
    }
    __syncthreads();
    const float x0 = (float)x0s[(wave * 32 + lr) * pF + h];
#pragma unroll
    for (int s = 0; s < kCinMaxH / 16; ++s) {
      if (16 * s < H) {                                     // (uniform)
        bf16x8 a;
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (bf16_t)(x0 * xr[s][j]);
#pragma unroll
        for (int t = 0; t < NTU; ++t) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(Ws + (32 * t + lr) * pw + 16 * s + 8 * hh);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
        }
      }
    }
  }
  // bias in fp32, one rounding; the pad columns U .. ldy - 1 are zeroed
#pragma unroll
  for (int t = 0; t < NTU; ++t) {
    const int o = 32 * t + lr;
    const float bo = o < U ? bias[o] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t r = row0 + wave * 32 + acc_row(i, hh);
      if (r < R && o < ldy) Y[r * ldy + o] = o < U ? (bf16_t)(acc[t][i] + bo) : bzero();
    }
  }
}

// ---------------------------------------------------------------- backward, inputs
// dx0t (fp32 [R, F]) = (accumulate ? dx0t : 0) + sum_m dA xi  (+ dxi for layer 1, whose xi IS x0t);
// otherwise dyprev[r, m] = bf16(dxi[r, m] + gpool[r / E, m]): the gradient of the layer below, rounded once.
template <int NTH>
__global__ void __launch_bounds__(256) cin_fused_bwd_input_kernel(
    const bf16_t* __restrict__ dY, int lddy, int U, const bf16_t* __restrict__ W, const bf16_t* __restrict__ x0t,
    int ld0, int F, const bf16_t* __restrict__ xi, int ldi, int H, int64_t R, float* __restrict__ dx0t, int accumulate,
    int first, const bf16_t* __restrict__ gpool, int64_t ldg, int E, bf16_t* __restrict__ dyprev, int ldp) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int Up = (U + 15) & ~15, pw = Up + 8, pF = F | 1, pD = F + 1, K = F * H;
  float* __restrict__ dxs = reinterpret_cast<float*>(smem);                       // [128][pD]: the tile's dx0t
  bf16_t* __restrict__ Wt = reinterpret_cast<bf16_t*>(dxs + kCinRows * pD);        // [NTH * 32][pw]: W[o, h*H + m] at [m][o]
  bf16_t* __restrict__ x0s = Wt + NTH * 32 * pw;                                   // [128][pF]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, hh = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * kCinRows, row = row0 + wave * 32 + lr;
  const bool valid = row < R;
  stage_x0(x0t, ld0, F, row0, R, x0s, pF);
  // B operand: dY[r, 16 s + 8 hh + j], kept for all fields
  bf16x8 dyf[kCinMaxH / 16];
#pragma unroll
  for (int s = 0; s < kCinMaxH / 16; ++s) {
    const int o0 = 16 * s + 8 * hh;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bzero();
    if (valid && o0 < lddy && 16 * s < U) v = *reinterpret_cast<const bf16x8*>(dY + row * lddy + o0);
#pragma unroll
    for (int j = 0; j < 8; ++j) dyf[s][j] = o0 + j < U ? v[j] : bzero();
  }
  // the row's xi in the accumulator's order: register i of tile t holds m = 32 t + acc_row(i, hh)
  float xr[NTH][16], dxi[NTH][16];
#pragma unroll
  for (int t = 0; t < NTH; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m0 = 32 * t + 8 * q + 4 * hh;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid && m0 < ldi) v = load4(xi + row * ldi + m0);
      xr[t][4 * q + 0] = m0 + 0 < H ? v.x : 0.f;
      xr[t][4 * q + 1] = m0 + 1 < H ? v.y : 0.f;
      xr[t][4 * q + 2] = m0 + 2 < H ? v.z : 0.f;
      xr[t][4 * q + 3] = m0 + 3 < H ? v.w : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) dxi[t][4 * q + e] = 0.f;
    }
  // The slice's element tid + 256 i sits at m = tid % (NTH * 32), o = tid / (NTH * 32) + i * (256 / (NTH * 32)); all
  // loads ahead of the barrier, as in the forward kernel.
  constexpr int MW = NTH * 32, NW = NTH * 16;               // NW * (256 / MW) = 128 >= Up
  const int wm = tid & (MW - 1), wo = tid / MW;
  bf16_t wv[NW];
  for (int h = 0; h < F; ++h) {
    const int base = h * H + wm;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int o = wo + i * (256 / MW);
      wv[i] = (o < U && wm < H) ? W[o * K + base] : bzero();          // (U * K <= 2^19)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int o = wo + i * (256 / MW);
      if (o < Up) Wt[wm * pw + o] = wv[i];
    }
    __syncthreads();
    f32x16 acc[NTH];
#pragma unroll
    for (int t = 0; t < NTH; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
#pragma unroll
    for (int s = 0; s < kCinMaxH / 16; ++s) {
      if (16 * s < U) {                                     // (uniform)
#pragma unroll
        for (int t = 0; t < NTH; ++t) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(Wt + (32 * t + lr) * pw + 16 * s + 8 * hh);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, dyf[s], acc[t], 0, 0, 0);
        }
      }
    }
    const float x0 = (float)x0s[(wave * 32 + lr) * pF + h];
    float p = 0.f;
#pragma unroll
    for (int t = 0; t < NTH; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        dxi[t][i] = fmaf(acc[t][i], x0, dxi[t][i]);
        p = fmaf(acc[t][i], xr[t][i], p);
      }
    p += __shfl_xor(p, 32, kWave);
    if (hh == 0) dxs[(wave * 32 + lr) * pD + h] = p;
  }
  __syncthreads();
  if (first) {                                              // layer 1: H == F, dxi joins the dx0t tile
#pragma unroll
    for (int t = 0; t < NTH; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = 32 * t + acc_row(i, hh);
        if (m < F) dxs[(wave * 32 + lr) * pD + m] += dxi[t][i];
      }
    __syncthreads();
  } else if (valid) {
    const int64_t b = row / E;
#pragma unroll
    for (int t = 0; t < NTH; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m0 = 32 * t + 8 * q + 4 * hh;
        if (m0 < ldp) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int m = m0 + e;
            v[e] = m < H ? dxi[t][4 * q + e] + (gpool ? (float)gpool[b * ldg + m] : 0.f) : 0.f;
          }
          store4(dyprev + row * ldp + m0, make_float4(v[0], v[1], v[2], v[3]));
        }
      }
  }
  const int col = tid & 63;
  if (col < F)
    for (int rr = tid >> 6; rr < kCinRows; rr += 4)
      if (row0 + rr < R) {
        float* __restrict__ g = dx0t + (row0 + rr) * F + col;
        const float v = dxs[rr * pD + col];
        *g = accumulate ? *g + v : v;
      }
}

// ---------------------------------------------------------------- backward, weights
// part[slab][o, h*H + m] = sum over the slab's rows of dY[r, o] * bf16(x0t[r, h] * xi[r, m]).
// grid (slabs, ceil(F * ceil(U / 32) / 8)); wave w of a workgroup owns item (h, ot) = blockIdx.y * 8 + w.
template <int NTH>
__global__ void __launch_bounds__(512) cin_fused_bwd_weight_kernel(const bf16_t* __restrict__ dY, int lddy, int U,
                                                                   const bf16_t* __restrict__ x0t, int ld0, int F,
                                                                   const bf16_t* __restrict__ xi, int ldi, int H,
                                                                   int64_t R, int64_t slab_rows,
                                                                   float* __restrict__ part) {
  __shared__ __align__(16) bf16_t dYt[kCinMaxH * kDwPitch];          // [o][row of the chunk]
  __shared__ __align__(16) bf16_t xit[kCinMaxH * kDwPitch];          // [m][row]
  __shared__ __align__(16) bf16_t x0tt[kCinMaxF * kDwPitch];         // [h][row]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, hh = lane >> 5;
  const int ntu = (U + 31) >> 5, item = blockIdx.y * 8 + wave;
  const bool active = item < F * ntu;
  const int h = active ? item / ntu : 0, ot = active ? item - h * ntu : 0;
  for (int i = tid; i < kCinMaxH * kDwPitch; i += 512) {
    dYt[i] = bzero();
    xit[i] = bzero();
    if (i < kCinMaxF * kDwPitch) x0tt[i] = bzero();
  }
  f32x16 acc[NTH];
#pragma unroll
  for (int t = 0; t < NTH; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  const int64_t rbeg = (int64_t)blockIdx.x * slab_rows, rend = rbeg + slab_rows < R ? rbeg + slab_rows : R;
  const int rr = tid >> 3, sub = tid & 7;
  for (int64_t r0 = rbeg; r0 < rend; r0 += kDwChunk) {
    __syncthreads();
    const int64_t row = r0 + rr;
    const bool ok = row < rend;
    // 8 consecutive columns per load (every pitch is a multiple of 8), written transposed; rows behind the slab: zeros
    auto stage = [&](const bf16_t* __restrict__ src, int ld, int n, bf16_t* __restrict__ dst) {
      for (int c0 = 8 * sub; c0 < n; c0 += 64) {
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bzero();
        if (ok) v = *reinterpret_cast<const bf16x8*>(src + row * ld + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (c0 + e < n) dst[(c0 + e) * kDwPitch + rr] = v[e];
      }
    };
    stage(dY, lddy, U, dYt);
    stage(xi, ldi, H, xit);
    stage(x0t, ld0, F, x0tt);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int ks = 0; ks < kDwChunk / 16; ++ks) {
        const int rb = 16 * ks + 8 * hh;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(dYt + (32 * ot + lr) * kDwPitch + rb);
        const bf16x8 x0v = *reinterpret_cast<const bf16x8*>(x0tt + h * kDwPitch + rb);
#pragma unroll
        for (int t = 0; t < NTH; ++t) {
          const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xit + (32 * t + lr) * kDwPitch + rb);
          bf16x8 b;
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] = (bf16_t)((float)x0v[j] * (float)xv[j]);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  const int64_t K = (int64_t)F * H;
  float* __restrict__ dst = part + (int64_t)blockIdx.x * U * K;
#pragma unroll
  for (int t = 0; t < NTH; ++t) {
    const int m = 32 * t + lr;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = 32 * ot + acc_row(i, hh);
      if (o < U && m < H) dst[o * K + h * H + m] = acc[t][i];
    }
  }
}

// dw[i] = part[0][i] + part[1][i] + ...  (slab order)
__global__ void __launch_bounds__(256) cin_slab_sum_kernel(const float* __restrict__ part, int64_t n, int slabs,
                                                           float* __restrict__ dw) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float s = part[i];
    for (int k = 1; k < slabs; ++k) s += part[k * n + i];
    dw[i] = s;
  }
}

// ---------------------------------------------------------------- glue, bf16 I/O forms of cin.hip's
// out[(b*C + c) * ld + r] = x[b, r, c]  (r < Rr; zeros up to ld)
__global__ void __launch_bounds__(256) cin_transpose_bf16_kernel(const bf16_t* __restrict__ x, int64_t B, int Rr, int C,
                                                                 bf16_t* __restrict__ out, int ld) {
  const int64_t per = (int64_t)C * ld, n = B * per;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / per;
    const int o = (int)(t - b * per);
    const int c = o / ld, r = o - c * ld;
    out[t] = r < Rr ? x[(b * Rr + r) * C + c] : bzero();
  }
}

// dx3[b, f, d] = bf16(dx0t[(b*E + d) * F + f])
__global__ void __launch_bounds__(256) cin_dx3_bf16_kernel(const float* __restrict__ dx0t, int64_t B, int E, int F,
                                                           bf16_t* __restrict__ dx3) {
  const int64_t per = (int64_t)E * F, n = B * per;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / per;
    const int o = (int)(t - b * per);
    const int f = o / E, d = o - f * E;
    dx3[t] = (bf16_t)dx0t[b * per + (int64_t)d * F + f];
  }
}

// out[b * ld_out + o] = bf16(sum_d y[(b*E + d) * ldy + o]): fp32 sum of the stored rows, one rounding
__global__ void __launch_bounds__(256) cin_pool_fwd_bf16_kernel(const bf16_t* __restrict__ y, int ldy, int64_t B, int E,
                                                                int U, bf16_t* __restrict__ out, int64_t ld_out) {
  const int64_t n = B * U;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / U;
    const int o = (int)(t - b * U);
    float s = 0.f;
    for (int d = 0; d < E; ++d) s += (float)y[(b * E + d) * ldy + o];
    out[b * ld_out + o] = (bf16_t)s;
  }
}

// dy[(b*E + d) * ld + o] = g[b * ldg + o]  (the top layer's gradient: the pooled gradient alone; pad columns zeroed)
__global__ void __launch_bounds__(256) cin_pool_bwd_bf16_kernel(const bf16_t* __restrict__ g, int64_t ldg, int64_t B,
                                                                int E, int U, bf16_t* __restrict__ dy, int ld) {
  const int64_t per = (int64_t)E * ld, n = B * per;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / per;
    const int o = (int)((t - b * per) % ld);
    dy[t] = o < U ? g[b * ldg + o] : bzero();
  }
}

static int cin_slabs(int64_t R) {
  const int64_t s = ceil_div(R, kDwSlabRows);
  return (int)(s < 1 ? 1 : s > kDwMaxSlabs ? kDwMaxSlabs : s);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace mapx

#define MAPX_CIN_SHAPES(what, F, H, U)                                                                          \
  MAPX_REQUIRE((F) >= 2 && (F) <= mapx::kCinMaxF, what ": num_fields in 2..64 (F=%d)", (int)(F));             \
  MAPX_REQUIRE((H) >= 1 && (H) <= mapx::kCinMaxH && (U) >= 1 && (U) <= mapx::kCinMaxH,                        \
               what ": cin_layer_units in 1..128 (H=%d, U=%d)", (int)(H), (int)(U))
#define MAPX_CIN_PITCH(what, ld, n) \
  MAPX_REQUIRE((ld) >= (n) && (ld) % 8 == 0, what ": row pitches are multiples of 8 elements, at least the width")

extern "C" int mapx_cin_fused_dw_slab_rows(void) { return mapx::kDwSlabRows; }

extern "C" int mapx_cin_fused_fwd(const mapx_bf16* x0t, int ld_x0, int F, const mapx_bf16* xi, int ld_xi, int H,
                                  const mapx_bf16* w, const float* bias, int U, int64_t R, mapx_bf16* y, int ld_y,
                                  hipStream_t stream) {
  using namespace mapx;
  MAPX_CIN_SHAPES("cin_fused_fwd", F, H, U);
  MAPX_CIN_PITCH("cin_fused_fwd", ld_x0, F);
  MAPX_CIN_PITCH("cin_fused_fwd", ld_xi, H);
  MAPX_CIN_PITCH("cin_fused_fwd", ld_y, U);
  MAPX_REQUIRE(R >= 0 && R < (1LL << 37), "cin_fused_fwd: bad R");
  if (R == 0) return MAPX_OK;
  MAPX_REQUIRE(x0t && xi && w && bias && y, "cin_fused_fwd: null pointer");
  MAPX_REQUIRE(aligned16(x0t) && aligned16(xi) && aligned16(y), "cin_fused_fwd: 16-byte aligned activations");
  const int ntu = (U + 31) / 32 > 2 ? 4 : (U + 31) / 32;
  const size_t lds = 2 * ((size_t)ntu * 32 * (((H + 15) & ~15) + 8) + (size_t)kCinRows * (F | 1));   // <= 52 KB
  const dim3 grid((unsigned)ceil_div(R, kCinRows));
#define MAPX_CIN_FWD(N) \
  hipLaunchKernelGGL(cin_fused_fwd_kernel<N>, grid, dim3(256), lds, stream, hc(x0t), ld_x0, F, hc(xi), ld_xi, H, hc(w), \
                     bias, U, R, hm(y), ld_y)
  if (ntu == 1) MAPX_CIN_FWD(1);
  else if (ntu == 2) MAPX_CIN_FWD(2);
  else MAPX_CIN_FWD(4);
#undef MAPX_CIN_FWD
  return check_launch("cin_fused_fwd");
}

extern "C" int mapx_cin_fused_bwd_input(const mapx_bf16* dy, int ld_dy, int U, const mapx_bf16* w, const mapx_bf16* x0t,
                                        int ld_x0, int F, const mapx_bf16* xi, int ld_xi, int H, int64_t R, float* dx0t,
                                        int accumulate_x0, int first_layer, const mapx_bf16* gpool, int64_t ld_g, int E,
                                        mapx_bf16* dy_prev, int ld_prev, hipStream_t stream) {
  using namespace mapx;
  MAPX_CIN_SHAPES("cin_fused_bwd_input", F, H, U);
  MAPX_CIN_PITCH("cin_fused_bwd_input", ld_x0, F);
  MAPX_CIN_PITCH("cin_fused_bwd_input", ld_xi, H);
  MAPX_CIN_PITCH("cin_fused_bwd_input", ld_dy, U);
  MAPX_REQUIRE(R >= 0 && R < (1LL << 37), "cin_fused_bwd_input: bad R");
  if (first_layer) {
    MAPX_REQUIRE(H == F && !dy_prev && !gpool, "cin_fused_bwd_input: layer 1 has H == F and no layer below");
  } else {
    MAPX_CIN_PITCH("cin_fused_bwd_input", ld_prev, H);
    MAPX_REQUIRE(E >= 1 && R % E == 0 && (!gpool || ld_g >= H), "cin_fused_bwd_input: bad E / ld_g");
  }
  if (R == 0) return MAPX_OK;
  MAPX_REQUIRE(dy && w && x0t && xi && dx0t && (first_layer || dy_prev), "cin_fused_bwd_input: null pointer");
  MAPX_REQUIRE(aligned16(dy) && aligned16(xi) && (first_layer || aligned16(dy_prev)),
               "cin_fused_bwd_input: 16-byte aligned activations");
  const int nth = (H + 31) / 32 > 2 ? 4 : (H + 31) / 32;
  const size_t lds = 4 * (size_t)kCinRows * (F + 1) +
                     2 * ((size_t)nth * 32 * (((U + 15) & ~15) + 8) + (size_t)kCinRows * (F | 1));       // <= 85 KB
  static const hipError_t optin = allow_dynamic_lds(96 * 1024, cin_fused_bwd_input_kernel<1>,
                                                    cin_fused_bwd_input_kernel<2>, cin_fused_bwd_input_kernel<4>);
  MAPX_HIP(optin);
  const dim3 grid((unsigned)ceil_div(R, kCinRows));
#define MAPX_CIN_BWD(N)                                                                                             \
  hipLaunchKernelGGL(cin_fused_bwd_input_kernel<N>, grid, dim3(256), lds, stream, hc(dy), ld_dy, U, hc(w), hc(x0t), \
                     ld_x0, F, hc(xi), ld_xi, H, R, dx0t, accumulate_x0, first_layer, hc(gpool), ld_g, E,           \
                     hm(dy_prev), ld_prev)
  if (nth == 1) MAPX_CIN_BWD(1);
  else if (nth == 2) MAPX_CIN_BWD(2);
  else MAPX_CIN_BWD(4);
#undef MAPX_CIN_BWD
  return check_launch("cin_fused_bwd_input");
}

extern "C" size_t mapx_cin_fused_bwd_weight_workspace_bytes(int F, int H, int U, int64_t R) {
  if (F < 1 || H < 1 || U < 1 || R < 0) return 0;
  return (size_t)mapx::cin_slabs(R) * U * F * H * sizeof(float);
}

extern "C" int mapx_cin_fused_bwd_weight(const mapx_bf16* dy, int ld_dy, int U, const mapx_bf16* x0t, int ld_x0, int F,
                                         const mapx_bf16* xi, int ld_xi, int H, int64_t R, void* ws, size_t ws_bytes,
                                         float* dw, hipStream_t stream) {
  using namespace mapx;
  MAPX_CIN_SHAPES("cin_fused_bwd_weight", F, H, U);
  MAPX_CIN_PITCH("cin_fused_bwd_weight", ld_x0, F);
  MAPX_CIN_PITCH("cin_fused_bwd_weight", ld_xi, H);
  MAPX_CIN_PITCH("cin_fused_bwd_weight", ld_dy, U);
  MAPX_REQUIRE(R >= 0 && R < (1LL << 37), "cin_fused_bwd_weight: bad R");
  MAPX_REQUIRE(dw, "cin_fused_bwd_weight: null pointer");
  const int64_t n = (int64_t)U * F * H;
  if (R == 0) {
    MAPX_HIP(hipMemsetAsync(dw, 0, n * sizeof(float), stream));
    return MAPX_OK;
  }
  MAPX_REQUIRE(dy && x0t && xi && ws, "cin_fused_bwd_weight: null pointer");
  MAPX_REQUIRE(aligned16(dy) && aligned16(xi) && aligned16(x0t), "cin_fused_bwd_weight: 16-byte aligned activations");
  if (ws_bytes < mapx_cin_fused_bwd_weight_workspace_bytes(F, H, U, R)) {
    set_error("cin_fused_bwd_weight: workspace too small");
    return MAPX_EWORKSPACE;
  }
  const int slabs = cin_slabs(R);
  const int64_t slab_rows = ceil_div(ceil_div(R, slabs), kDwChunk) * kDwChunk;
  const int nth = (H + 31) / 32 > 2 ? 4 : (H + 31) / 32;
  const dim3 grid((unsigned)slabs, (unsigned)ceil_div((int64_t)F * ((U + 31) / 32), 8));
  float* part = static_cast<float*>(ws);
#define MAPX_CIN_DW(N)                                                                                           \
  hipLaunchKernelGGL(cin_fused_bwd_weight_kernel<N>, grid, dim3(512), 0, stream, hc(dy), ld_dy, U, hc(x0t), ld_x0, F, \
                     hc(xi), ld_xi, H, R, slab_rows, part)
  if (nth == 1) MAPX_CIN_DW(1);
  else if (nth == 2) MAPX_CIN_DW(2);
  else MAPX_CIN_DW(4);
#undef MAPX_CIN_DW
  int rc = check_launch("cin_fused_bwd_weight");
  if (rc != MAPX_OK) return rc;
  hipLaunchKernelGGL(cin_slab_sum_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, part, n, slabs, dw);
  return check_launch("cin_slab_sum");
}

extern "C" int mapx_cin_transpose_bf16(const mapx_bf16* x, int64_t B, int R, int C, mapx_bf16* out, int ld_out,
                                       hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 0 && R > 0 && C > 0 && ld_out >= R, "cin_transpose_bf16: bad sizes");
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(x && out, "cin_transpose_bf16: null pointer");
  hipLaunchKernelGGL(cin_transpose_bf16_kernel, dim3(grid_for(B * C * ld_out, 256)), dim3(256), 0, stream, hc(x), B, R,
                     C, hm(out), ld_out);
  return check_launch("cin_transpose_bf16");
}

extern "C" int mapx_cin_dx3_bf16(const float* dx0t, int64_t B, int E, int F, mapx_bf16* dx3, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 0 && E > 0 && F > 0, "cin_dx3_bf16: bad sizes");
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(dx0t && dx3, "cin_dx3_bf16: null pointer");
  hipLaunchKernelGGL(cin_dx3_bf16_kernel, dim3(grid_for(B * E * F, 256)), dim3(256), 0, stream, dx0t, B, E, F, hm(dx3));
  return check_launch("cin_dx3_bf16");
}

extern "C" int mapx_cin_pool_fwd_bf16(const mapx_bf16* y, int ld_y, int64_t B, int E, int U, mapx_bf16* out,
                                      int64_t ld_out, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 0 && E > 0 && U > 0 && ld_y >= U && ld_out >= U, "cin_pool_fwd_bf16: bad sizes");
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(y && out, "cin_pool_fwd_bf16: null pointer");
  hipLaunchKernelGGL(cin_pool_fwd_bf16_kernel, dim3(grid_for(B * U, 256)), dim3(256), 0, stream, hc(y), ld_y, B, E, U,
                     hm(out), ld_out);
  return check_launch("cin_pool_fwd_bf16");
}

extern "C" int mapx_cin_pool_bwd_bf16(const mapx_bf16* g, int64_t ld_g, int64_t B, int E, int U, mapx_bf16* dy,
                                      int ld_dy, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 0 && E > 0 && U > 0 && ld_g >= U && ld_dy >= U, "cin_pool_bwd_bf16: bad sizes");
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(g && dy, "cin_pool_bwd_bf16: null pointer");
  hipLaunchKernelGGL(cin_pool_bwd_bf16_kernel, dim3(grid_for(B * E * ld_dy, 256)), dim3(256), 0, stream, hc(g), ld_g, B,
                     E, U, hm(dy), ld_dy);
  return check_launch("cin_pool_bwd_bf16");
}
