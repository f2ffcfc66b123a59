// FGCNN backbone (reference code/models.py:325-407, code/layers.py:204-251 FGCNNBlock, :105-137 InnerProductLayer
// output="inner_product"): Conv2d (kh x 1) -> BatchNorm2d -> tanh | relu -> MaxPool2d (ps x 1), and the pairwise
// inner products of the combined feature rows.  Every tensor [B, C, H, E] dense, E % 4 == 0.  The activations are
// T = float | bf16_t (common.h load4 / store4: a load widens, a store rounds to nearest even once); all arithmetic, the
// LDS contents, the parameters, the statistics, g = dL/du and every parameter gradient are fp32 (fp64 partials) in both
// forms.  With T = bf16_t the batch statistics are those of the STORED z (the rounded values widened back), the tensor
// that pool_fwd, pool_bwd and conv_bwd recompute xhat from: sum(xhat) stays 0 and the conv-bias gradient an fp32-level
// quantity.
//
// Conv forward.  One workgroup per sample: the weights [Cout, Cin, kh] and the sample's input slab [Cin, H, E] sit in
// LDS, one wave per output channel (channels dealt round robin to the 4 waves), lanes over (h, 4 columns of E).  The
// same launch leaves, per (sample, channel), the sum and the sum of squares of the channel's H*E outputs as fp64
// partials [B, Cout, 2]: z*z is exact in fp64, so E[z^2] - E[z]^2 formed in fp64 by the finalise kernel loses nothing
// an fp32 two-pass would keep.  bn_stats (one workgroup per channel) sums the partials in a fixed order, writes
// {mean, rstd} and moves the running statistics (unbiased variance, n / (n-1)) and the int64 batch counter on the
// device.
//
// BN + activation + max-pool forward is elementwise over the pooled tensor: u = gamma * (z - mean) * rstd + beta,
// a = act(u), y = max over the window rows o*ps - pad .. o*ps - pad + ps - 1 inside [0, H) (pad = H % ps rows of -inf
// on both ends, floor mode; the first of equal maxima wins), idx = the winner's position inside the window (uint8):
// the only tensor saved beside z.
//
// Backward.  pool_bwd (per sample, wave per channel) scatters dy through idx, multiplies by act'(u) recomputed from z
// and writes g = dL/du [B, C, H, E] with the fp64 partials of sum(g) and sum(g * xhat); bn_bwd_sums reduces them in a
// fixed order (dbeta, dgamma); conv_bwd (a fixed group of kConvBwdGroup samples per workgroup) forms
// dz = gamma * rstd * (g - dbeta/n - xhat * dgamma/n) in LDS and from it dX, and the group's partial dW / db, which
// conv_dw_sum adds up in a fixed order.  No atomics anywhere: a replay repeats every sum bit for bit.
//
// Inner product.  One workgroup per sample, its [T, E] rows in LDS at a pitch of E+4 floats; out[b, p] over the pairs
// i < j in row-major order (torch.masked_select with the strict upper-triangle mask).  Backward stages the sample's
// gradient row in LDS too: dx_i = sum_{j>i} g_ij x_j + sum_{j<i} g_ji x_j.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr int kFgMaxC = 32, kFgMaxKh = 15, kFgBlock = 256, kFgWaves = kFgBlock / kWave;
constexpr int kConvBwdGroup = 4;               // samples per workgroup of conv_bwd (one partial dW row per group)
constexpr int kIpMaxT = 192, kIpMaxE = 64;
constexpr size_t kFgLdsLimit = 128 * 1024;     // dynamic LDS the kernels may ask for (the CU has 160 KB)
enum { kActTanh = 0, kActRelu = 1 };

// THE normalised value and pre-activation of an element: forward and backward call these, so a relu unit sits on
// the same side of the kink in both.
__device__ inline float bn_xhat(float z, float mean, float rstd) { return __fmul_rn(__fsub_rn(z, mean), rstd); }
__device__ inline float bn_u(float xh, float ga, float be) { return __fmaf_rn(xh, ga, be); }
// (relu written so that a NaN stays one, as torch.relu keeps it)
__device__ inline float act_of(float u, int act) { return act == kActRelu ? (u <= 0.f ? 0.f : u) : tanhf(u); }
__device__ inline float act_grad(float u, int act) {
  if (act == kActRelu) return u > 0.f ? 1.f : 0.f;
  const float t = tanhf(u);
  return 1.f - t * t;
}

// ------------------------------------------------------------------------------------------------ conv forward
// What a store4 to T leaves in memory, as fp32.
__device__ inline float4 stored_as(const float*, const float4& v) { return v; }
__device__ inline float4 stored_as(const bf16_t*, const float4& v) {
  return make_float4((float)(bf16_t)v.x, (float)(bf16_t)v.y, (float)(bf16_t)v.z, (float)(bf16_t)v.w);
}

template <typename T>
__global__ void __launch_bounds__(kFgBlock) fgcnn_conv_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int Cin, int Cout, int H,
    int E, int kh, T* __restrict__ z, double* __restrict__ part) {
  extern __shared__ float sm[];
  const int nw = Cout * Cin * kh, nw4 = (nw + 3) / 4 * 4, E4 = E / 4, items = H * E4, pad = (kh - 1) / 2;
  float* sw = sm;                                            // [Cout][Cin][kh]
  float4* sx = reinterpret_cast<float4*>(sm + nw4);          // [Cin][H][E4]
  const int64_t b = blockIdx.x;
  for (int t = threadIdx.x; t < nw; t += kFgBlock) sw[t] = w[t];
  const T* xs = x + b * Cin * H * E;
  for (int t = threadIdx.x; t < Cin * items; t += kFgBlock) sx[t] = load4(xs + 4 * t);
  __syncthreads();
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (int co = wave; co < Cout; co += kFgWaves) {
    const float bc = bias[co];
    T* zo = z + (b * Cout + co) * H * E;
    double s = 0.0, ss = 0.0;
    for (int it = lane; it < items; it += kWave) {
      const int h = it / E4, e4 = it - h * E4;
      float4 acc = make_float4(bc, bc, bc, bc);
      const int k0 = max(0, pad - h), k1 = min(kh, H + pad - h);      // rows h + k - pad inside [0, H)
      for (int ci = 0; ci < Cin; ++ci) {
        const float* wr = sw + (co * Cin + ci) * kh;
        const float4* xr = sx + (ci * H + h - pad) * E4 + e4;
        for (int k = k0; k < k1; ++k) fma4(acc, wr[k], xr[k * E4]);
      }
      store4(zo + 4 * it, acc);
      acc = stored_as(zo, acc);                  // the statistics describe the stored tensor
      const double a0 = acc.x, a1 = acc.y, a2 = acc.z, a3 = acc.w;
      s += (a0 + a1) + (a2 + a3);
      ss += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    if (part) {
      s = group_sum<kWave>(s);
      ss = group_sum<kWave>(ss);
      if (lane == 0) {
        part[(b * Cout + co) * 2 + 0] = s;
        part[(b * Cout + co) * 2 + 1] = ss;
      }
    }
  }
}

// Sum of part[b][c][0..1] over b in a fixed order: thread t takes b = t, t + 256, ..., then an LDS tree.
__device__ inline void channel_totals(const double* __restrict__ part, int64_t B, int C, int c, double* sh,
                                      double& s0, double& s1) {
  double a = 0.0, q = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += kFgBlock) {
    a += part[(b * C + c) * 2 + 0];
    q += part[(b * C + c) * 2 + 1];
  }
  sh[threadIdx.x] = a;
  sh[kFgBlock + threadIdx.x] = q;
  __syncthreads();
  for (int o = kFgBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[threadIdx.x] += sh[threadIdx.x + o];
      sh[kFgBlock + threadIdx.x] += sh[kFgBlock + threadIdx.x + o];
    }
    __syncthreads();
  }
  s0 = sh[0];
  s1 = sh[kFgBlock];
}

__global__ void __launch_bounds__(kFgBlock) fgcnn_bn_stats_kernel(const double* __restrict__ part, int64_t B, int C,
                                                                  double n, float eps, float momentum,
                                                                  float* __restrict__ stats,
                                                                  float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var,
                                                                  int64_t* __restrict__ tracked) {
  __shared__ double sh[2 * kFgBlock];
  const int c = blockIdx.x;
  double s, ss;
  channel_totals(part, B, C, c, sh, s, ss);
  if (threadIdx.x == 0) {
    const double mean = s / n;
    double var = ss / n - mean * mean;           // biased; fp64 over exact squares
    if (var < 0.0) var = 0.0;
    stats[2 * c + 0] = (float)mean;
    stats[2 * c + 1] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
      const float unbiased = (float)(var * n / (n - 1.0));
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
    if (c == 0 && tracked) *tracked += 1;
  }
}

// ------------------------------------------------------------------------------------------------ BN + act + pool
template <typename T>
__global__ void __launch_bounds__(kFgBlock) fgcnn_pool_fwd_kernel(
    const T* __restrict__ z, const float* __restrict__ stats, const float* __restrict__ running_mean,
    const float* __restrict__ running_var, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
    int64_t total4, int C, int H, int E4, int ps, int pad, int Hp, int act, T* __restrict__ y,
    uint8_t* __restrict__ idx) {
  for (int64_t t = (int64_t)blockIdx.x * kFgBlock + threadIdx.x; t < total4; t += (int64_t)gridDim.x * kFgBlock) {
    const int e4 = (int)(t % E4);
    const int64_t r = t / E4;
    const int o = (int)(r % Hp);
    const int64_t bc = r / Hp;
    const int c = (int)(bc % C);
    float mean, rstd;
    if (stats) {
      mean = stats[2 * c];
      rstd = stats[2 * c + 1];
    } else {
      mean = running_mean[c];
      rstd = 1.0f / sqrtf(running_var[c] + eps);
    }
    const float ga = gamma[c], be = beta[c];
    const T* zr = z + (bc * H * E4 + e4) * 4;
    const float ninf = -__builtin_huge_valf();
    float4 best = make_float4(ninf, ninf, ninf, ninf);
    uchar4 bi = make_uchar4(0, 0, 0, 0);
    const int h0 = o * ps - pad;
    for (int k = 0; k < ps; ++k) {
      const int h = h0 + k;
      if (h < 0 || h >= H) continue;
      const float4 v = load4(zr + (int64_t)h * E4 * 4);
      const float a0 = act_of(bn_u(bn_xhat(v.x, mean, rstd), ga, be), act);
      const float a1 = act_of(bn_u(bn_xhat(v.y, mean, rstd), ga, be), act);
      const float a2 = act_of(bn_u(bn_xhat(v.z, mean, rstd), ga, be), act);
      const float a3 = act_of(bn_u(bn_xhat(v.w, mean, rstd), ga, be), act);
      // (torch's rule: a NaN wins and stays, so a diverged run does not look finite behind the pooling)
      if (a0 > best.x || a0 != a0) { best.x = a0; bi.x = (uint8_t)k; }
      if (a1 > best.y || a1 != a1) { best.y = a1; bi.y = (uint8_t)k; }
      if (a2 > best.z || a2 != a2) { best.z = a2; bi.z = (uint8_t)k; }
      if (a3 > best.w || a3 != a3) { best.w = a3; bi.w = (uint8_t)k; }
    }
    store4(y + t * 4, best);
    if (idx) reinterpret_cast<uchar4*>(idx)[t] = bi;
  }
}

template <typename T>
__global__ void __launch_bounds__(kFgBlock) fgcnn_pool_bwd_kernel(
    const T* __restrict__ dy, const uint8_t* __restrict__ idx, const T* __restrict__ z,
    const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta, int C, int H,
    int E, int ps, int pad, int Hp, int act, float* __restrict__ g, double* __restrict__ part) {
  const int E4 = E / 4, items = H * E4;
  const int64_t b = blockIdx.x;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (int c = wave; c < C; c += kFgWaves) {
    const float mean = stats[2 * c], rstd = stats[2 * c + 1], ga = gamma[c], be = beta[c];
    const int64_t bc = b * C + c;
    const T* zr = z + bc * items * 4;
    float4* gr = reinterpret_cast<float4*>(g) + bc * items;
    const T* dyr = dy + bc * Hp * E4 * 4;
    const uchar4* ir = reinterpret_cast<const uchar4*>(idx) + bc * Hp * E4;
    double s = 0.0, sx = 0.0;
    for (int it = lane; it < items; it += kWave) {
      const int h = it / E4, e4 = it - h * E4;
      const int o = (h + pad) / ps, k = (h + pad) - o * ps;
      const float4 v = load4(zr + 4 * it);
      const float x0 = bn_xhat(v.x, mean, rstd), x1 = bn_xhat(v.y, mean, rstd), x2 = bn_xhat(v.z, mean, rstd),
                  x3 = bn_xhat(v.w, mean, rstd);
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (o < Hp) {
        const float4 d = load4(dyr + (o * E4 + e4) * 4);
        const uchar4 iv = ir[o * E4 + e4];
        if (iv.x == k) gv.x = d.x * act_grad(bn_u(x0, ga, be), act);
        if (iv.y == k) gv.y = d.y * act_grad(bn_u(x1, ga, be), act);
        if (iv.z == k) gv.z = d.z * act_grad(bn_u(x2, ga, be), act);
        if (iv.w == k) gv.w = d.w * act_grad(bn_u(x3, ga, be), act);
      }
      gr[it] = gv;
      const double g0 = gv.x, g1 = gv.y, g2 = gv.z, g3 = gv.w;
      s += (g0 + g1) + (g2 + g3);
      sx += (g0 * x0 + g1 * x1) + (g2 * x2 + g3 * x3);
    }
    s = group_sum<kWave>(s);
    sx = group_sum<kWave>(sx);
    if (lane == 0) {
      part[bc * 2 + 0] = s;
      part[bc * 2 + 1] = sx;
    }
  }
}

__global__ void __launch_bounds__(kFgBlock) fgcnn_bn_bwd_sums_kernel(const double* __restrict__ part, int64_t B, int C,
                                                                     double n, float* __restrict__ bsum,
                                                                     float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta) {
  __shared__ double sh[2 * kFgBlock];
  const int c = blockIdx.x;
  double s, sx;
  channel_totals(part, B, C, c, sh, s, sx);
  if (threadIdx.x == 0) {
    bsum[2 * c + 0] = (float)(s / n);
    bsum[2 * c + 1] = (float)(sx / n);
    dbeta[c] = (float)s;
    dgamma[c] = (float)sx;
  }
}

// ------------------------------------------------------------------------------------------------ conv backward
template <typename T>
__global__ void __launch_bounds__(kFgBlock) fgcnn_conv_bwd_kernel(
    const float* __restrict__ g, const T* __restrict__ z, const T* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ bsum, int64_t B, int Cin,
    int Cout, int H, int E, int kh, T* __restrict__ dx, float* __restrict__ pw, float* __restrict__ pb) {
  extern __shared__ float sm[];
  const int nw = Cout * Cin * kh, nw4 = (nw + 3) / 4 * 4, E4 = E / 4, items = H * E4, pad = (kh - 1) / 2;
  float* sw = sm;                                                    // [Cout][Cin][kh]
  float4* sx = reinterpret_cast<float4*>(sm + nw4);                  // [Cin][H][E4]
  float4* sd = sx + Cin * items;                                     // [Cout][H][E4]: dz
  for (int t = threadIdx.x; t < nw; t += kFgBlock) sw[t] = w[t];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float* pwr = pw + (int64_t)blockIdx.x * nw;
  float* pbr = pb + (int64_t)blockIdx.x * Cout;
  for (int sidx = 0; sidx < kConvBwdGroup; ++sidx) {
    const int64_t b = (int64_t)blockIdx.x * kConvBwdGroup + sidx;
    if (b >= B) break;                                               // (uniform over the workgroup)
    __syncthreads();                                                 // the previous sample's slabs are free
    const T* xs = x + b * Cin * items * 4;
    for (int t = threadIdx.x; t < Cin * items; t += kFgBlock) sx[t] = load4(xs + 4 * t);
    const float4* gs = reinterpret_cast<const float4*>(g) + b * Cout * items;
    const T* zs = z + b * Cout * items * 4;
    for (int t = threadIdx.x; t < Cout * items; t += kFgBlock) {
      const int co = t / items;
      const float mean = stats[2 * co], rstd = stats[2 * co + 1], sc = gamma[co] * rstd;
      const float mb = bsum[2 * co], mg = bsum[2 * co + 1];
      const float4 gv = gs[t], zv = load4(zs + 4 * t);
      float4 d;
      d.x = sc * ((gv.x - mb) - bn_xhat(zv.x, mean, rstd) * mg);
      d.y = sc * ((gv.y - mb) - bn_xhat(zv.y, mean, rstd) * mg);
      d.z = sc * ((gv.z - mb) - bn_xhat(zv.z, mean, rstd) * mg);
      d.w = sc * ((gv.w - mb) - bn_xhat(zv.w, mean, rstd) * mg);
      sd[t] = d;
    }
    __syncthreads();
    // dX[ci, h] = sum_co sum_k w[co, ci, k] dz[co, h - k + pad]
    if (dx) {
      T* dxs = dx + b * Cin * items * 4;
      for (int t = threadIdx.x; t < Cin * items; t += kFgBlock) {
        const int ci = t / items, it = t - ci * items, h = it / E4, e4 = it - h * E4;
        const int k0 = max(0, h + pad - (H - 1)), k1 = min(kh, h + pad + 1);      // rows h - k + pad inside [0, H)
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int co = 0; co < Cout; ++co) {
          const float* wr = sw + (co * Cin + ci) * kh;
          const float4* dr = sd + (co * H + h + pad) * E4 + e4;
          for (int k = k0; k < k1; ++k) fma4(acc, wr[k], dr[-k * E4]);
        }
        store4(dxs + 4 * t, acc);
      }
    }
    // dW[co, ci, k] += sum_h dz[co, h] . x[ci, h + k - pad]: every entry has one owner thread, which adds the
    // group's samples in order into the group's partial row
    for (int t = threadIdx.x; t < nw; t += kFgBlock) {
      const int k = t % kh, cc = t / kh, ci = cc % Cin, co = cc / Cin;
      const int h0 = max(0, pad - k), h1 = min(H, H + pad - k);
      const float4* dr = sd + co * items;
      const float4* xr = sx + ci * items + (k - pad) * E4;
      float acc = 0.f;
      for (int i = h0 * E4; i < h1 * E4; ++i) acc = dot4(dr[i], xr[i], acc);
      pwr[t] = sidx == 0 ? acc : pwr[t] + acc;
    }
    // db[co] += sum dz[co]
    for (int co = wave; co < Cout; co += kFgWaves) {
      float acc = 0.f;
      for (int it = lane; it < items; it += kWave) {
        const float4 d = sd[co * items + it];
        acc += (d.x + d.y) + (d.z + d.w);
      }
      acc = group_sum<kWave>(acc);
      if (lane == 0) pbr[co] = sidx == 0 ? acc : pbr[co] + acc;
    }
  }
}

// dw[i] = sum over the groups' partial rows, in order; thread per entry (entries [0, nw) = dW, [nw, nw + Cout) = db).
__global__ void __launch_bounds__(kFgBlock) fgcnn_conv_dw_sum_kernel(const float* __restrict__ pw,
                                                                     const float* __restrict__ pb, int64_t G, int nw,
                                                                     int Cout, float* __restrict__ dw,
                                                                     float* __restrict__ db) {
  const int i = blockIdx.x * kFgBlock + threadIdx.x;
  if (i >= nw + Cout) return;
  const bool is_w = i < nw;
  const float* src = is_w ? pw + i : pb + (i - nw);
  const int64_t ld = is_w ? nw : Cout;
  // four interleaved chains (a fixed order) keep the loads in flight; the rows are added in fp64
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t r = 0;
  for (; r + 4 <= G; r += 4) {
    a0 += src[(r + 0) * ld];
    a1 += src[(r + 1) * ld];
    a2 += src[(r + 2) * ld];
    a3 += src[(r + 3) * ld];
  }
  for (; r < G; ++r) a0 += src[r * ld];
  const float s = (float)((a0 + a1) + (a2 + a3));
  if (is_w) dw[i] = s;
  else db[i - nw] = s;
}

// ------------------------------------------------------------------------------------------------ inner product
__device__ inline int ip_row_offset(int i, int T) { return i * (2 * T - i - 1) / 2; }      // pairs before row i

// (a bf16 output row of the generally odd width T(T-1)/2 is only 2-byte aligned: one element per store in both forms)
template <typename S>
__global__ void __launch_bounds__(kFgBlock) inner_product_fwd_kernel(const S* __restrict__ x, int T, int E,
                                                                     S* __restrict__ out) {
  extern __shared__ float sm[];
  const int E4 = E / 4, LD4 = E4 + 1;                   // row pitch E + 4 floats
  float4* sx = reinterpret_cast<float4*>(sm);
  const int64_t b = blockIdx.x;
  const S* xs = x + b * T * E4 * 4;
  for (int t = threadIdx.x; t < T * E4; t += kFgBlock) sx[(t / E4) * LD4 + t % E4] = load4(xs + 4 * t);
  __syncthreads();
  const int64_t P = (int64_t)T * (T - 1) / 2;
  S* o = out + b * P;
  // Row i of the triangle has T-1-i pairs: rows r and T-2-r folded into one line of T slots, so every trip of the
  // loop is a pair (the middle row of an odd count stands alone).
  const int R = T - 1, lines = (R + 1) / 2;
  for (int t = threadIdx.x; t < lines * T; t += kFgBlock) {
    const int r = t / T, c = t - r * T, len = T - 1 - r;
    int i, j;
    if (c < len) {
      i = r;
      j = r + 1 + c;
    } else {
      i = R - 1 - r;
      if (i == r) continue;
      j = i + 1 + (c - len);
    }
    float acc = 0.f;
    for (int c = 0; c < E4; ++c) acc = dot4(sx[i * LD4 + c], sx[j * LD4 + c], acc);
    o[ip_row_offset(i, T) + j - i - 1] = (S)acc;
  }
}

// g: rows of T(T-1)/2 elements at a pitch of ldg elements (a column slice of a wider gradient is read in place).
template <typename S>
__global__ void __launch_bounds__(kFgBlock) inner_product_bwd_kernel(const S* __restrict__ g, int64_t ldg,
                                                                     const S* __restrict__ x, int T, int E,
                                                                     S* __restrict__ dx) {
  extern __shared__ float sm[];
  const int E4 = E / 4, LD4 = E4 + 1;
  const int P = T * (T - 1) / 2, P4 = (P + 3) / 4 * 4;
  float* sg = sm;                                       // [P]
  float4* sx = reinterpret_cast<float4*>(sm + P4);      // [T][LD4]
  const int64_t b = blockIdx.x;
  const S* gs = g + b * ldg;
  for (int t = threadIdx.x; t < P; t += kFgBlock) sg[t] = (float)gs[t];
  const S* xs = x + b * T * E4 * 4;
  for (int t = threadIdx.x; t < T * E4; t += kFgBlock) sx[(t / E4) * LD4 + t % E4] = load4(xs + 4 * t);
  __syncthreads();
  S* dxs = dx + b * T * E4 * 4;
  for (int t = threadIdx.x; t < T * E4; t += kFgBlock) {
    const int i = t / E4, c = t - i * E4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < i; ++j) fma4(acc, sg[ip_row_offset(j, T) + i - j - 1], sx[j * LD4 + c]);
    const float* gi = sg + ip_row_offset(i, T) - i - 1;
    for (int j = i + 1; j < T; ++j) fma4(acc, gi[j], sx[j * LD4 + c]);
    store4(dxs + 4 * t, acc);
  }
}

static hipError_t raise_lds_limit() {
  // (the opt-in above 64 KB is per instantiation)
  static const hipError_t done = allow_dynamic_lds(
      kFgLdsLimit, &fgcnn_conv_fwd_kernel<float>, &fgcnn_conv_bwd_kernel<float>, &inner_product_fwd_kernel<float>,
      &inner_product_bwd_kernel<float>, &fgcnn_conv_fwd_kernel<bf16_t>, &fgcnn_conv_bwd_kernel<bf16_t>,
      &inner_product_fwd_kernel<bf16_t>, &inner_product_bwd_kernel<bf16_t>);
  return done;
}

static int conv_shape_check(const char* what, int64_t B, int Cin, int Cout, int H, int E, int kh, size_t lds) {
  MAPX_REQUIRE(B >= 0 && B < (1LL << 31), "%s: bad batch size", what);
  MAPX_REQUIRE(Cin >= 1 && Cin <= kFgMaxC && Cout >= 1 && Cout <= kFgMaxC,
               "%s: 1..%d channels (got Cin=%d Cout=%d)", what, kFgMaxC, Cin, Cout);
  MAPX_REQUIRE(kh >= 1 && kh <= kFgMaxKh && kh % 2 == 1, "%s: odd kernel height <= %d (got %d)", what, kFgMaxKh, kh);
  MAPX_REQUIRE(H >= 1 && E >= 4 && E % 4 == 0, "%s: H >= 1 rows of E %% 4 == 0 columns (got H=%d E=%d)", what, H, E);
  MAPX_REQUIRE(lds <= kFgLdsLimit, "%s: weights and one sample's slabs take %zu bytes of LDS, above %zu "
               "(Cin=%d Cout=%d H=%d E=%d kh=%d)", what, lds, kFgLdsLimit, Cin, Cout, H, E, kh);
  return MAPX_OK;
}

static int pool_shape_check(const char* what, int64_t B, int C, int H, int E, int ps, int* pad, int* Hp) {
  MAPX_REQUIRE(B >= 0 && B < (1LL << 31) && C >= 1 && C <= kFgMaxC && H >= 1 && E >= 4 && E % 4 == 0,
               "%s: 1..%d channels, H >= 1 rows of E %% 4 == 0 columns (got C=%d H=%d E=%d)", what, kFgMaxC, C, H, E);
  MAPX_REQUIRE(ps >= 1 && ps <= 255, "%s: pooling size 1..255 (got %d)", what, ps);
  *pad = H % ps;
  MAPX_REQUIRE(2 * *pad <= ps, "%s: pooling padding H %% ps = %d is more than half of the pooling size %d "
               "(torch's MaxPool2d raises too: pad should be at most half of the kernel size)", what, *pad, ps);
  *Hp = (H + 2 * *pad - ps) / ps + 1;
  MAPX_REQUIRE(H + 2 * *pad >= ps && *Hp >= 1, "%s: H=%d rows are fewer than one pooling window of %d", what, H, ps);
  return MAPX_OK;
}

template <typename T>
static int conv_fwd(const T* x, const float* w, const float* bias, int64_t B, int Cin, int Cout, int H, int E, int kh,
                    T* z, double* part_opt, hipStream_t stream) {
  const size_t lds = ((size_t)(Cout * Cin * kh + 3) / 4 * 4 + (size_t)Cin * H * E) * sizeof(float);
  if (int rc = conv_shape_check("fgcnn_conv_fwd", B, Cin, Cout, H, E, kh, lds)) return rc;
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(x && w && bias && z, "fgcnn_conv_fwd: null pointer");
  MAPX_HIP(raise_lds_limit());
  hipLaunchKernelGGL(fgcnn_conv_fwd_kernel<T>, dim3((unsigned)B), dim3(kFgBlock), lds, stream, x, w, bias, Cin, Cout, H,
                     E, kh, z, part_opt);
  return check_launch("fgcnn_conv_fwd");
}

template <typename T>
static int pool_fwd(const T* z, const float* stats_opt, const float* running_mean_opt, const float* running_var_opt,
                    float eps, const float* gamma, const float* beta, int64_t B, int C, int H, int E, int ps, int act,
                    T* y, uint8_t* idx_opt, hipStream_t stream) {
  int pad, Hp;
  if (int rc = pool_shape_check("fgcnn_pool_fwd", B, C, H, E, ps, &pad, &Hp)) return rc;
  MAPX_REQUIRE(act == kActTanh || act == kActRelu, "fgcnn_pool_fwd: activation 0 (tanh) | 1 (relu), got %d", act);
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(z && gamma && beta && y && (stats_opt || (running_mean_opt && running_var_opt)),
               "fgcnn_pool_fwd: null pointer");
  const int64_t total4 = B * C * Hp * (E / 4);
  hipLaunchKernelGGL(fgcnn_pool_fwd_kernel<T>, dim3(grid_for(total4, kFgBlock)), dim3(kFgBlock), 0, stream, z,
                     stats_opt, running_mean_opt, running_var_opt, eps, gamma, beta, total4, C, H, E / 4, ps, pad, Hp,
                     act, y, idx_opt);
  return check_launch("fgcnn_pool_fwd");
}

template <typename T>
static int pool_bwd(const T* dy, const uint8_t* idx, const T* z, const float* stats, const float* gamma,
                    const float* beta, int64_t B, int C, int H, int E, int ps, int act, float* g, double* part,
                    hipStream_t stream) {
  int pad, Hp;
  if (int rc = pool_shape_check("fgcnn_pool_bwd", B, C, H, E, ps, &pad, &Hp)) return rc;
  MAPX_REQUIRE(act == kActTanh || act == kActRelu, "fgcnn_pool_bwd: activation 0 (tanh) | 1 (relu), got %d", act);
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(dy && idx && z && stats && gamma && beta && g && part, "fgcnn_pool_bwd: null pointer");
  hipLaunchKernelGGL(fgcnn_pool_bwd_kernel<T>, dim3((unsigned)B), dim3(kFgBlock), 0, stream, dy, idx, z, stats, gamma,
                     beta, C, H, E, ps, pad, Hp, act, g, part);
  return check_launch("fgcnn_pool_bwd");
}

template <typename T>
static int conv_bwd(const float* g, const T* z, const T* x, const float* w, const float* stats, const float* gamma,
                    const float* bsum, int64_t B, int Cin, int Cout, int H, int E, int kh, T* dx_opt, float* part_w,
                    float* part_b, float* dw, float* db, hipStream_t stream) {
  const size_t lds = ((size_t)(Cout * Cin * kh + 3) / 4 * 4 + (size_t)(Cin + Cout) * H * E) * sizeof(float);
  if (int rc = conv_shape_check("fgcnn_conv_bwd", B, Cin, Cout, H, E, kh, lds)) return rc;
  MAPX_REQUIRE(B >= 1, "fgcnn_conv_bwd: empty batch");
  MAPX_REQUIRE(g && z && x && w && stats && gamma && bsum && part_w && part_b && dw && db,
               "fgcnn_conv_bwd: null pointer");
  MAPX_HIP(raise_lds_limit());
  const int G = (int)ceil_div(B, kConvBwdGroup), nw = Cout * Cin * kh;
  hipLaunchKernelGGL(fgcnn_conv_bwd_kernel<T>, dim3((unsigned)G), dim3(kFgBlock), lds, stream, g, z, x, w, stats, gamma,
                     bsum, B, Cin, Cout, H, E, kh, dx_opt, part_w, part_b);
  if (int rc = check_launch("fgcnn_conv_bwd")) return rc;
  hipLaunchKernelGGL(fgcnn_conv_dw_sum_kernel, dim3((unsigned)ceil_div(nw + Cout, kFgBlock)), dim3(kFgBlock), 0, stream,
                     part_w, part_b, (int64_t)G, nw, Cout, dw, db);
  return check_launch("fgcnn_conv_dw_sum");
}

static int ip_shape_check(const char* what, int64_t B, int T, int E) {
  MAPX_REQUIRE(B >= 0 && B < (1LL << 31), "%s: bad batch size", what);
  MAPX_REQUIRE(T >= 2 && T <= kIpMaxT, "%s: 2..%d feature rows (got T=%d)", what, kIpMaxT, T);
  MAPX_REQUIRE(E >= 4 && E % 4 == 0 && E <= kIpMaxE, "%s: row width E %% 4 == 0, <= %d (got %d)", what, kIpMaxE, E);
  return MAPX_OK;
}

template <typename S>
static int ip_fwd(const S* x, int64_t B, int T, int E, S* out, hipStream_t stream) {
  if (int rc = ip_shape_check("inner_product_fwd", B, T, E)) return rc;
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(x && out, "inner_product_fwd: null pointer");
  MAPX_HIP(raise_lds_limit());
  const size_t lds = (size_t)T * (E + 4) * sizeof(float);
  hipLaunchKernelGGL(inner_product_fwd_kernel<S>, dim3((unsigned)B), dim3(kFgBlock), lds, stream, x, T, E, out);
  return check_launch("inner_product_fwd");
}

template <typename S>
static int ip_bwd(const S* g, int64_t ldg, const S* x, int64_t B, int T, int E, S* dx, hipStream_t stream) {
  if (int rc = ip_shape_check("inner_product_bwd", B, T, E)) return rc;
  MAPX_REQUIRE(ldg >= (int64_t)T * (T - 1) / 2, "inner_product_bwd: the gradient's row pitch %lld is below its width "
               "T(T-1)/2 = %d", (long long)ldg, T * (T - 1) / 2);
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(g && x && dx, "inner_product_bwd: null pointer");
  MAPX_HIP(raise_lds_limit());
  const size_t lds = ((size_t)(T * (T - 1) / 2 + 3) / 4 * 4 + (size_t)T * (E + 4)) * sizeof(float);
  hipLaunchKernelGGL(inner_product_bwd_kernel<S>, dim3((unsigned)B), dim3(kFgBlock), lds, stream, g, ldg, x, T, E, dx);
  return check_launch("inner_product_bwd");
}

}  // namespace mapx

extern "C" int mapx_fgcnn_conv_fwd(const float* x, const float* w, const float* bias, int64_t B, int Cin, int Cout,
                                   int H, int E, int kh, float* z, double* part_opt, hipStream_t stream) {
  return mapx::conv_fwd(x, w, bias, B, Cin, Cout, H, E, kh, z, part_opt, stream);
}

extern "C" int mapx_fgcnn_conv_fwd_bf16(const mapx_bf16* x, const float* w, const float* bias, int64_t B, int Cin,
                                        int Cout, int H, int E, int kh, mapx_bf16* z, double* part_opt,
                                        hipStream_t stream) {
  return mapx::conv_fwd(mapx::hc(x), w, bias, B, Cin, Cout, H, E, kh, mapx::hm(z), part_opt, stream);
}

extern "C" int mapx_fgcnn_bn_stats(const double* part, int64_t B, int C, int H, int E, float eps, float momentum,
                                   float* stats, float* running_mean_opt, float* running_var_opt,
                                   int64_t* num_batches_tracked_opt, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 1 && C >= 1 && C <= kFgMaxC && H >= 1 && E >= 1, "fgcnn_bn_stats: bad shape");
  MAPX_REQUIRE((double)B * H * E > 1.0, "fgcnn_bn_stats: batch statistics need more than one value per channel "
               "(B=%lld H=%d E=%d)", (long long)B, H, E);
  MAPX_REQUIRE(part && stats && (!running_mean_opt == !running_var_opt), "fgcnn_bn_stats: null pointer");
  hipLaunchKernelGGL(fgcnn_bn_stats_kernel, dim3((unsigned)C), dim3(kFgBlock), 0, stream, part, B, C,
                     (double)B * H * E, eps, momentum, stats, running_mean_opt, running_var_opt,
                     num_batches_tracked_opt);
  return check_launch("fgcnn_bn_stats");
}

extern "C" int mapx_fgcnn_pool_fwd(const float* z, const float* stats_opt, const float* running_mean_opt,
                                   const float* running_var_opt, float eps, const float* gamma, const float* beta,
                                   int64_t B, int C, int H, int E, int ps, int act, float* y, uint8_t* idx_opt,
                                   hipStream_t stream) {
  return mapx::pool_fwd(z, stats_opt, running_mean_opt, running_var_opt, eps, gamma, beta, B, C, H, E, ps, act, y,
                        idx_opt, stream);
}

extern "C" int mapx_fgcnn_pool_fwd_bf16(const mapx_bf16* z, const float* stats_opt, const float* running_mean_opt,
                                        const float* running_var_opt, float eps, const float* gamma, const float* beta,
                                        int64_t B, int C, int H, int E, int ps, int act, mapx_bf16* y, uint8_t* idx_opt,
                                        hipStream_t stream) {
  return mapx::pool_fwd(mapx::hc(z), stats_opt, running_mean_opt, running_var_opt, eps, gamma, beta, B, C, H, E, ps,
                        act, mapx::hm(y), idx_opt, stream);
}

extern "C" int mapx_fgcnn_pool_bwd(const float* dy, const uint8_t* idx, const float* z, const float* stats,
                                   const float* gamma, const float* beta, int64_t B, int C, int H, int E, int ps,
                                   int act, float* g, double* part, hipStream_t stream) {
  return mapx::pool_bwd(dy, idx, z, stats, gamma, beta, B, C, H, E, ps, act, g, part, stream);
}

extern "C" int mapx_fgcnn_pool_bwd_bf16(const mapx_bf16* dy, const uint8_t* idx, const mapx_bf16* z, const float* stats,
                                        const float* gamma, const float* beta, int64_t B, int C, int H, int E, int ps,
                                        int act, float* g, double* part, hipStream_t stream) {
  return mapx::pool_bwd(mapx::hc(dy), idx, mapx::hc(z), stats, gamma, beta, B, C, H, E, ps, act, g, part, stream);
}

extern "C" int mapx_fgcnn_bn_bwd_sums(const double* part, int64_t B, int C, int H, int E, float* bsum, float* dgamma,
                                      float* dbeta, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 1 && C >= 1 && C <= kFgMaxC && H >= 1 && E >= 1, "fgcnn_bn_bwd_sums: bad shape");
  MAPX_REQUIRE(part && bsum && dgamma && dbeta, "fgcnn_bn_bwd_sums: null pointer");
  hipLaunchKernelGGL(fgcnn_bn_bwd_sums_kernel, dim3((unsigned)C), dim3(kFgBlock), 0, stream, part, B, C,
                     (double)B * H * E, bsum, dgamma, dbeta);
  return check_launch("fgcnn_bn_bwd_sums");
}

extern "C" int mapx_fgcnn_conv_bwd_groups(int64_t B) {
  return (int)((B + mapx::kConvBwdGroup - 1) / mapx::kConvBwdGroup);
}

extern "C" int mapx_fgcnn_conv_bwd(const float* g, const float* z, const float* x, const float* w, const float* stats,
                                   const float* gamma, const float* bsum, int64_t B, int Cin, int Cout, int H, int E,
                                   int kh, float* dx_opt, float* part_w, float* part_b, float* dw, float* db,
                                   hipStream_t stream) {
  return mapx::conv_bwd(g, z, x, w, stats, gamma, bsum, B, Cin, Cout, H, E, kh, dx_opt, part_w, part_b, dw, db, stream);
}

extern "C" int mapx_fgcnn_conv_bwd_bf16(const float* g, const mapx_bf16* z, const mapx_bf16* x, const float* w,
                                        const float* stats, const float* gamma, const float* bsum, int64_t B, int Cin,
                                        int Cout, int H, int E, int kh, mapx_bf16* dx_opt, float* part_w, float* part_b,
                                        float* dw, float* db, hipStream_t stream) {
  return mapx::conv_bwd(g, mapx::hc(z), mapx::hc(x), w, stats, gamma, bsum, B, Cin, Cout, H, E, kh, mapx::hm(dx_opt),
                        part_w, part_b, dw, db, stream);
}

extern "C" int mapx_inner_product_fwd(const float* x, int64_t B, int T, int E, float* out, hipStream_t stream) {
  return mapx::ip_fwd(x, B, T, E, out, stream);
}

extern "C" int mapx_inner_product_bwd(const float* g, const float* x, int64_t B, int T, int E, float* dx,
                                      hipStream_t stream) {
  return mapx::ip_bwd(g, (int64_t)T * (T - 1) / 2, x, B, T, E, dx, stream);
}

extern "C" int mapx_inner_product_fwd_bf16(const mapx_bf16* x, int64_t B, int T, int E, mapx_bf16* out,
                                           hipStream_t stream) {
  return mapx::ip_fwd(mapx::hc(x), B, T, E, mapx::hm(out), stream);
}

extern "C" int mapx_inner_product_bwd_bf16(const mapx_bf16* g, int64_t ldg, const mapx_bf16* x, int64_t B, int T, int E,
                                           mapx_bf16* dx, hipStream_t stream) {
  return mapx::ip_bwd(mapx::hc(g), ldg, mapx::hc(x), B, T, E, mapx::hm(dx), stream);
}
