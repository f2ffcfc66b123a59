// FiGNN backbone (reference code/layers.py:300-379 GraphLayer / FiGNNBlock / AttentionalPrediction, code/models.py:
// 410-438).  Everything fp32; x and every h are [B, F, E] dense, E % 4 == 0, E <= 32, 2 <= F <= 64.  A sample's whole
// state is a few KB: the work is row-resident, not a GEMM call.
//
// Graph.  One wave per sample (four samples per workgroup, x rows in LDS at a pitch of E+4 floats): lane i forms
// s_i = w_src . x_i and d_i = w_dst . x_i, then row i of the graph is one pass over the lanes j: pre = s_i + d_j,
// Leaky-ReLU (slope 0.01), the diagonal masked, a wave-wide max / sum softmax.  g [B,F,F] (g_ii = 0 exactly), s and d
// [B,F] are written; backward recomputes pre from s and d, so it sits on the same side of the kink.
//
// Layer.  A workgroup walks a tile of samples.  The GRU's two [3E,E] matrices and its biases always sit in LDS (pitch
// E+4); W_in and W_out [F,E,E] too when they fit next to the tile in 80 KB (two workgroups per CU), else they are
// streamed through L2.  Per sample, with one owner thread per (field, column): h_out_i = W_out[i] h_i, aggr = g h_out,
// a_i = W_in[i] aggr_i + bias_p, the GRU cell (gates r, z, n as torch orders them) and the optional residual.  Nothing
// but the layer's output is kept: backward re-runs the very same device function on the saved input h and g, then
// walks back: gate gradients, da, the direct dh, d_aggr = W_in^T da, dg (+)= d_aggr h_out^T, dh_out = g^T d_aggr,
// dh += W_out^T dh_out, and with res_conn the running dx (+)= dh'.  The vectors the weight gradients need
// (a, aggr, da, dh_out and the four gate gradients, 8 E floats per row) go to a workspace; two kernels form per-chunk
// partial sums from it (per field over 64 samples for dW_in / dW_out, over 64 rows for the GRU pair, its biases and
// bias_p), and a finalise kernel adds the chunks in a fixed order in fp64, eight interleaved row slices per column
// (overwriting, or adding to what an earlier layer left: the shared GRU, reuse_graph_layer).  No atomics: a replay repeats every sum bit for bit.
//
// Graph backward.  Wave per sample: dalpha = g (dg - sum_j g dg), times the Leaky-ReLU slope, row sums ds and column
// sums dd, dx_i = base_i (+ add_i) + ds_i w_src + dd_i w_dst; dW_attn from per-wave partial rows.
//
// Prediction.  logits_b = sum_f sigmoid(z2_bf) score_bf and its two input gradients.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr int kGnBlock = 256, kGnWaves = kGnBlock / kWave;
constexpr int kGnMaxF = 64, kGnMaxE = 32;
constexpr size_t kGnLdsLimit = 128 * 1024;     // dynamic LDS a layer kernel may ask for (the CU has 160 KB)
// W_in / W_out are staged only while two workgroups still share a CU's LDS: at F = 23, E = 16 the forward kernel (75 KB
// staged) ran 0.33 ms per three layers against 0.52 streamed, the backward kernel (82 KB staged, one workgroup per CU)
// 1.47 against 1.19 streamed at 23.5 KB
constexpr size_t kGnStageLimit = 80 * 1024;
constexpr float kGnLeaky = 0.01f;
constexpr int kGnFieldChunk = 64;              // samples per partial row of dW_in / dW_out
constexpr int kGnGruChunk = 64;                // (sample, field) rows per partial row of the GRU's gradients
constexpr int kGnMaxTile = 32;                 // samples a workgroup of a layer kernel walks at most
// workspace vectors per (sample, field) row, E floats each
enum { kWsA = 0, kWsAggr = 1, kWsDa = 2, kWsDho = 3, kWsDr = 4, kWsDz = 5, kWsDn = 6, kWsDhn = 7, kWsVecs = 8 };

// One v_fmac_f32 per term, by hand, as in skinny.hip: several dot products that run side by side over LDS operands
// (s and d of the graph, the GRU's six gates) are otherwise paired into v_pk_fma_f32 whose low lane takes the high
// half of a ds_read result — the form tools/isa_guard.py keeps out of every kernel that ships.
static __device__ inline float gn_dot4(const float4& a, const float4& b, float s) {
  asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(s) : "v"(a.x), "v"(b.x));
  asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(s) : "v"(a.y), "v"(b.y));
  asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(s) : "v"(a.z), "v"(b.z));
  asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(s) : "v"(a.w), "v"(b.w));
  return s;
}

static __device__ inline float gn_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// ------------------------------------------------------------------------------------------------ graph
__global__ void __launch_bounds__(kGnBlock) fignn_graph_fwd_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ wa, int64_t B, int F, int E,
                                                                   float* __restrict__ g, float* __restrict__ s,
                                                                   float* __restrict__ d) {
  extern __shared__ float sm[];
  const int EP = E + 4, E4 = E / 4;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float* sx = sm + wave * F * EP;
  const float4* wsrc = reinterpret_cast<const float4*>(wa);
  const float4* wdst = reinterpret_cast<const float4*>(wa + E);
  for (int64_t b0 = (int64_t)blockIdx.x * kGnWaves; b0 < B; b0 += (int64_t)gridDim.x * kGnWaves) {
    const int64_t b = b0 + wave;
    const bool valid = b < B;                                      // (uniform over the wave)
    __syncthreads();                                               // the previous sample's rows are free
    if (valid) {
      const float4* xs = reinterpret_cast<const float4*>(x + b * F * E);
      for (int t = lane; t < F * E4; t += kWave) {
        const int i = t / E4, c = t - i * E4;
        reinterpret_cast<float4*>(sx + i * EP)[c] = xs[t];
      }
    }
    __syncthreads();
    if (!valid) continue;
    float si = 0.f, di = 0.f;
    if (lane < F) {
      const float4* xr = reinterpret_cast<const float4*>(sx + lane * EP);
      for (int c = 0; c < E4; ++c) {
        const float4 xv = xr[c];
        si = gn_dot4(wsrc[c], xv, si);
        di = gn_dot4(wdst[c], xv, di);
      }
      s[b * F + lane] = si;
      d[b * F + lane] = di;
    }
    for (int i = 0; i < F; ++i) {
      const float pre = __shfl(si, i, kWave) + di;
      const float al = pre > 0.f ? pre : kGnLeaky * pre;
      const bool on = lane < F && lane != i;
      const float m = group_max<kWave>(on ? al : -__builtin_huge_valf());
      const float p = on ? expf(al - m) : 0.f;
      const float sum = group_sum<kWave>(p);
      if (lane < F) g[(b * F + i) * F + lane] = p / sum;
    }
  }
}

// (dx may be base itself: every element is read and then written by one thread)
__global__ void __launch_bounds__(kGnBlock) fignn_graph_bwd_kernel(
    const float* __restrict__ dg, const float* __restrict__ g, const float* __restrict__ s, const float* __restrict__ d,
    const float* __restrict__ x, const float* __restrict__ wa, const float* base, const float* __restrict__ add,
    int64_t B, int F, int E, float* dx, float* __restrict__ part) {
  extern __shared__ float sm[];
  const int EP = E + 4, E4 = E / 4;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float* sx = sm + wave * (F * EP + 2 * kWave);
  float* sds = sx + F * EP;
  float* sdd = sds + kWave;
  const float4* wsrc = reinterpret_cast<const float4*>(wa);
  const float4* wdst = reinterpret_cast<const float4*>(wa + E);
  float wacc = 0.f;                    // lane l < 2E: column l of dW_attn over this wave's samples, in order
  for (int64_t b0 = (int64_t)blockIdx.x * kGnWaves; b0 < B; b0 += (int64_t)gridDim.x * kGnWaves) {
    const int64_t b = b0 + wave;
    const bool valid = b < B;
    __syncthreads();
    if (valid) {
      const float4* xs = reinterpret_cast<const float4*>(x + b * F * E);
      for (int t = lane; t < F * E4; t += kWave) {
        const int i = t / E4, c = t - i * E4;
        reinterpret_cast<float4*>(sx + i * EP)[c] = xs[t];
      }
      const float sl = lane < F ? s[b * F + lane] : 0.f;
      const float dj = lane < F ? d[b * F + lane] : 0.f;
      float ds_i = 0.f, dd_j = 0.f;
      for (int i = 0; i < F; ++i) {
        float gv = 0.f, dgv = 0.f;
        if (lane < F) {
          gv = g[(b * F + i) * F + lane];
          dgv = dg[(b * F + i) * F + lane];
        }
        const float rd = group_sum<kWave>(gv * dgv);
        const float pre = __shfl(sl, i, kWave) + dj;
        float dp = gv * (dgv - rd);                                // (g = 0 on the diagonal and past F)
        dp = pre > 0.f ? dp : kGnLeaky * dp;
        dd_j += dp;
        const float rs = group_sum<kWave>(dp);
        if (lane == i) ds_i = rs;
      }
      sds[lane] = ds_i;
      sdd[lane] = dd_j;
    }
    __syncthreads();
    if (!valid) continue;
    const float4* bs = reinterpret_cast<const float4*>(base + b * F * E);
    const float4* as = add ? reinterpret_cast<const float4*>(add + b * F * E) : nullptr;
    float4* dxs = reinterpret_cast<float4*>(dx + b * F * E);
    for (int t = lane; t < F * E4; t += kWave) {
      const int i = t / E4, c = t - i * E4;
      float4 v = bs[t];
      if (as) {
        const float4 a = as[t];
        v.x += a.x;
        v.y += a.y;
        v.z += a.z;
        v.w += a.w;
      }
      fma4(v, sds[i], wsrc[c]);
      fma4(v, sdd[i], wdst[c]);
      dxs[t] = v;
    }
    if (lane < 2 * E) {
      const float* sv = lane < E ? sds : sdd;
      const int e = lane < E ? lane : lane - E;
      float acc = 0.f;
      for (int i = 0; i < F; ++i) acc = fmaf(sv[i], sx[i * EP + e], acc);
      wacc += acc;
    }
  }
  if (lane < 2 * E) part[((int64_t)blockIdx.x * kGnWaves + wave) * 2 * E + lane] = wacc;
}

// ------------------------------------------------------------------------------------------------ layer
// LDS of a layer kernel, in floats: the GRU block, the staged W_in / W_out, `nbuf` [F,E] sample buffers, g [F,F].
__host__ __device__ inline size_t gn_gru_floats(int E) { return (size_t)6 * E * (E + 4) + 7 * E; }
__host__ __device__ inline size_t gn_sample_floats(int F, int E, int nbuf) {
  return (size_t)nbuf * F * E + (size_t)(F * F + 3) / 4 * 4;
}
__host__ __device__ inline size_t gn_weight_floats(int F, int E) { return (size_t)2 * F * E * (E + 4); }
constexpr int kGnFwdBufs = 4, kGnBwdBufs = 9;

struct GnLds {
  float *wih, *whh, *bih, *bhh, *bp;     // [3E][E+4] x 2, [3E] x 2, [E]
  float *win, *wout;                     // [F][E][E+4] when staged
  float *h, *ho, *ag, *a, *r, *z, *n, *hn, *dh, *g;
};

static __device__ inline GnLds gn_carve(float* sm, int F, int E, bool staged, int nbuf) {
  GnLds L;
  const int EP = E + 4, FE = F * E;
  float* p = sm;
  L.wih = p; p += 3 * E * EP;
  L.whh = p; p += 3 * E * EP;
  L.bih = p; p += 3 * E;
  L.bhh = p; p += 3 * E;
  L.bp = p;  p += E;
  L.win = p; if (staged) p += (size_t)FE * EP;
  L.wout = p; if (staged) p += (size_t)FE * EP;
  L.h = p;  p += FE;
  L.ho = p; p += FE;
  L.ag = p; p += FE;
  L.a = p;  p += FE;
  // (the forward kernel asks for four sample buffers only and never touches the rest)
  L.r = p;  if (nbuf > 4) p += FE;
  L.z = p;  if (nbuf > 4) p += FE;
  L.n = p;  if (nbuf > 4) p += FE;
  L.hn = p; if (nbuf > 4) p += FE;
  L.dh = p; if (nbuf > 4) p += FE;
  L.g = p;
  return L;
}

// Weights into LDS: the GRU block always, W_in / W_out when STAGED.  (A __syncthreads() must follow.)
template <bool STAGED>
static __device__ inline void gn_stage_weights(const GnLds& L, const float* __restrict__ w_in,
                                               const float* __restrict__ w_out, const float* __restrict__ bias_p,
                                               const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                               const float* __restrict__ b_ih, const float* __restrict__ b_hh, int F,
                                               int E) {
  const int EP = E + 4, E4 = E / 4;
  for (int t = threadIdx.x; t < 3 * E * E4; t += kGnBlock) {
    const int row = t / E4, c = t - row * E4;
    reinterpret_cast<float4*>(L.wih + row * EP)[c] = reinterpret_cast<const float4*>(w_ih)[t];
    reinterpret_cast<float4*>(L.whh + row * EP)[c] = reinterpret_cast<const float4*>(w_hh)[t];
  }
  for (int t = threadIdx.x; t < 3 * E; t += kGnBlock) {
    L.bih[t] = b_ih[t];
    L.bhh[t] = b_hh[t];
  }
  for (int t = threadIdx.x; t < E; t += kGnBlock) L.bp[t] = bias_p[t];
  if (STAGED) {
    for (int t = threadIdx.x; t < F * E * E4; t += kGnBlock) {
      const int row = t / E4, c = t - row * E4;
      reinterpret_cast<float4*>(L.win + (size_t)row * EP)[c] = reinterpret_cast<const float4*>(w_in)[t];
      reinterpret_cast<float4*>(L.wout + (size_t)row * EP)[c] = reinterpret_cast<const float4*>(w_out)[t];
    }
  }
}

// Row (i, e) of a per-field matrix: LDS at pitch E+4 when staged, else global at pitch E.
template <bool STAGED>
static __device__ inline const float* gn_wrow(const float* lds, const float* __restrict__ glob, int row, int E) {
  return STAGED ? lds + (size_t)row * (E + 4) : glob + (size_t)row * E;
}

// THE forward of one sample, on L.h and L.g (loaded, and a barrier passed): leaves h_out, aggr and a in L.ho / L.ag /
// L.a.  KEEP (backward): r, z, n and W_hn h + b_hn go to L.r / L.z / L.n / L.hn; else h' (+ xres) goes to `hnext`.
template <bool STAGED, bool KEEP>
static __device__ inline void gn_forward_sample(const GnLds& L, const float* __restrict__ w_in,
                                                const float* __restrict__ w_out, int F, int E,
                                                const float* __restrict__ xres, float* __restrict__ hnext) {
  const int FE = F * E, E4 = E / 4, EP = E + 4;
  for (int o = threadIdx.x; o < FE; o += kGnBlock) {
    const int i = o / E;
    const float4* w4 = reinterpret_cast<const float4*>(gn_wrow<STAGED>(L.wout, w_out, o, E));
    const float4* v4 = reinterpret_cast<const float4*>(L.h + i * E);
    float acc = 0.f;
    for (int c = 0; c < E4; ++c) acc = gn_dot4(w4[c], v4[c], acc);
    L.ho[o] = acc;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < FE; o += kGnBlock) {
    const int i = o / E, e = o - i * E;
    const float* gr = L.g + i * F;
    float acc = 0.f;
    for (int j = 0; j < F; ++j) acc = fmaf(gr[j], L.ho[j * E + e], acc);
    L.ag[o] = acc;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < FE; o += kGnBlock) {
    const int i = o / E, e = o - i * E;
    const float4* w4 = reinterpret_cast<const float4*>(gn_wrow<STAGED>(L.win, w_in, o, E));
    const float4* v4 = reinterpret_cast<const float4*>(L.ag + i * E);
    float acc = 0.f;
    for (int c = 0; c < E4; ++c) acc = gn_dot4(w4[c], v4[c], acc);
    L.a[o] = acc + L.bp[e];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < FE; o += kGnBlock) {
    const int i = o / E, e = o - i * E;
    const float4* a4 = reinterpret_cast<const float4*>(L.a + i * E);
    const float4* h4 = reinterpret_cast<const float4*>(L.h + i * E);
    const float4* ir4 = reinterpret_cast<const float4*>(L.wih + e * EP);
    const float4* iz4 = reinterpret_cast<const float4*>(L.wih + (E + e) * EP);
    const float4* in4 = reinterpret_cast<const float4*>(L.wih + (2 * E + e) * EP);
    const float4* hr4 = reinterpret_cast<const float4*>(L.whh + e * EP);
    const float4* hz4 = reinterpret_cast<const float4*>(L.whh + (E + e) * EP);
    const float4* hn4 = reinterpret_cast<const float4*>(L.whh + (2 * E + e) * EP);
    float ir = L.bih[e], iz = L.bih[E + e], in = L.bih[2 * E + e];
    float hr = L.bhh[e], hz = L.bhh[E + e], hn = L.bhh[2 * E + e];
    for (int c = 0; c < E4; ++c) {
      const float4 av = a4[c], hv = h4[c];
      ir = gn_dot4(ir4[c], av, ir);
      iz = gn_dot4(iz4[c], av, iz);
      in = gn_dot4(in4[c], av, in);
      hr = gn_dot4(hr4[c], hv, hr);
      hz = gn_dot4(hz4[c], hv, hz);
      hn = gn_dot4(hn4[c], hv, hn);
    }
    const float r = gn_sigmoid(ir + hr), z = gn_sigmoid(iz + hz);
    const float n = tanhf(fmaf(r, hn, in));
    if (KEEP) {
      L.r[o] = r;
      L.z[o] = z;
      L.n[o] = n;
      L.hn[o] = hn;
    } else {
      float hp = fmaf(z, L.h[o] - n, n);                           // (1 - z) n + z h
      if (xres) hp += xres[o];
      hnext[o] = hp;
    }
  }
}

static __device__ inline void gn_load_sample(const GnLds& L, const float* __restrict__ h, const float* __restrict__ g,
                                             int64_t b, int F, int E) {
  const int FE4 = F * E / 4;
  const float4* hs = reinterpret_cast<const float4*>(h + b * F * E);
  for (int t = threadIdx.x; t < FE4; t += kGnBlock) reinterpret_cast<float4*>(L.h)[t] = hs[t];
  const float* gs = g + b * F * F;
  for (int t = threadIdx.x; t < F * F; t += kGnBlock) L.g[t] = gs[t];
}

template <bool STAGED>
__global__ void __launch_bounds__(kGnBlock) fignn_layer_fwd_kernel(
    const float* __restrict__ h, const float* __restrict__ g, const float* __restrict__ xres,
    const float* __restrict__ w_in, const float* __restrict__ w_out, const float* __restrict__ bias_p,
    const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
    const float* __restrict__ b_hh, int64_t B, int S, int F, int E, float* __restrict__ hnext) {
  extern __shared__ float sm[];
  const GnLds L = gn_carve(sm, F, E, STAGED, kGnFwdBufs);
  gn_stage_weights<STAGED>(L, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh, F, E);
  for (int sidx = 0; sidx < S; ++sidx) {
    const int64_t b = (int64_t)blockIdx.x * S + sidx;
    if (b >= B) break;                                             // (uniform over the workgroup)
    __syncthreads();                                               // weights staged / the previous sample is done
    gn_load_sample(L, h, g, b, F, E);
    __syncthreads();
    gn_forward_sample<STAGED, false>(L, w_in, w_out, F, E, xres ? xres + b * F * E : nullptr, hnext + b * F * E);
  }
}

template <bool STAGED>
__global__ void __launch_bounds__(kGnBlock) fignn_layer_bwd_kernel(
    const float* __restrict__ dhn, const float* __restrict__ h, const float* __restrict__ g,
    const float* __restrict__ w_in, const float* __restrict__ w_out, const float* __restrict__ bias_p,
    const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
    const float* __restrict__ b_hh, int64_t B, int S, int F, int E, float* __restrict__ dh, float* __restrict__ dg,
    int dg_init, float* __restrict__ dxacc, int dx_init, float* __restrict__ ws) {
  extern __shared__ float sm[];
  const GnLds L = gn_carve(sm, F, E, STAGED, kGnBwdBufs);
  const int FE = F * E, EP = E + 4, E4 = E / 4;
  gn_stage_weights<STAGED>(L, w_in, w_out, bias_p, w_ih, w_hh, b_ih, b_hh, F, E);
  for (int sidx = 0; sidx < S; ++sidx) {
    const int64_t b = (int64_t)blockIdx.x * S + sidx;
    if (b >= B) break;
    __syncthreads();
    gn_load_sample(L, h, g, b, F, E);
    __syncthreads();
    gn_forward_sample<STAGED, true>(L, w_in, w_out, F, E, nullptr, nullptr);
    __syncthreads();
    float* wsb = ws + b * FE * kWsVecs;
    // gate gradients (each thread rewrites its own r, z, n, hn slots with them)
    for (int o = threadIdx.x; o < FE; o += kGnBlock) {
      const int i = o / E, e = o - i * E;
      const float dhp = dhn[b * FE + o];
      const float r = L.r[o], z = L.z[o], n = L.n[o], hn = L.hn[o], hv = L.h[o];
      const float dnp = dhp * (1.f - z) * (1.f - n * n);
      const float dzp = dhp * (hv - n) * z * (1.f - z);
      const float drp = dnp * hn * r * (1.f - r);
      const float dhnp = dnp * r;
      L.r[o] = drp;
      L.z[o] = dzp;
      L.n[o] = dnp;
      L.hn[o] = dhnp;
      L.dh[o] = dhp * z;
      if (dxacc) dxacc[b * FE + o] = dx_init ? dhp : dxacc[b * FE + o] + dhp;
      float* wr = wsb + i * kWsVecs * E + e;
      wr[kWsA * E] = L.a[o];
      wr[kWsAggr * E] = L.ag[o];
      wr[kWsDr * E] = drp;
      wr[kWsDz * E] = dzp;
      wr[kWsDn * E] = dnp;
      wr[kWsDhn * E] = dhnp;
    }
    __syncthreads();
    // da = W_ih^T dgi (into L.a), dh = dh' z + W_hh^T dgh (in L.dh)
    for (int o = threadIdx.x; o < FE; o += kGnBlock) {
      const int i = o / E, k = o - i * E;
      float da = 0.f, dhh = L.dh[o];
      for (int e = 0; e < E; ++e) {
        const float drp = L.r[i * E + e], dzp = L.z[i * E + e], dnp = L.n[i * E + e], dhnp = L.hn[i * E + e];
        da = fmaf(L.wih[e * EP + k], drp, da);
        da = fmaf(L.wih[(E + e) * EP + k], dzp, da);
        da = fmaf(L.wih[(2 * E + e) * EP + k], dnp, da);
        dhh = fmaf(L.whh[e * EP + k], drp, dhh);
        dhh = fmaf(L.whh[(E + e) * EP + k], dzp, dhh);
        dhh = fmaf(L.whh[(2 * E + e) * EP + k], dhnp, dhh);
      }
      L.a[o] = da;
      L.dh[o] = dhh;
      wsb[(i * kWsVecs + kWsDa) * E + k] = da;
    }
    __syncthreads();
    // d_aggr_i = W_in[i]^T da_i (into L.ag)
    for (int o = threadIdx.x; o < FE; o += kGnBlock) {
      const int i = o / E, k = o - i * E;
      float acc = 0.f;
      for (int e = 0; e < E; ++e) acc = fmaf(gn_wrow<STAGED>(L.win, w_in, i * E + e, E)[k], L.a[i * E + e], acc);
      L.ag[o] = acc;
    }
    __syncthreads();
    // dg (+)= d_aggr h_out^T;  dh_out = g^T d_aggr (into L.n)
    float* dgb = dg + b * F * F;
    for (int t = threadIdx.x; t < F * F; t += kGnBlock) {
      const int i = t / F, j = t - i * F;
      const float4* p4 = reinterpret_cast<const float4*>(L.ag + i * E);
      const float4* q4 = reinterpret_cast<const float4*>(L.ho + j * E);
      float acc = 0.f;
      for (int c = 0; c < E4; ++c) acc = gn_dot4(p4[c], q4[c], acc);
      dgb[t] = dg_init ? acc : dgb[t] + acc;
    }
    for (int o = threadIdx.x; o < FE; o += kGnBlock) {
      const int j = o / E, e = o - j * E;
      float acc = 0.f;
      for (int i = 0; i < F; ++i) acc = fmaf(L.g[i * F + j], L.ag[i * E + e], acc);
      L.n[o] = acc;
      wsb[(j * kWsVecs + kWsDho) * E + e] = acc;
    }
    __syncthreads();
    // dh_i += W_out[i]^T dh_out_i
    for (int o = threadIdx.x; o < FE; o += kGnBlock) {
      const int i = o / E, k = o - i * E;
      float acc = L.dh[o];
      for (int e = 0; e < E; ++e) acc = fmaf(gn_wrow<STAGED>(L.wout, w_out, i * E + e, E)[k], L.n[i * E + e], acc);
      dh[b * FE + o] = acc;
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradients
// Field i, chunk c of 64 samples: part[c][{W_in, W_out}][i][e][k] = sum_b {da, dh_out}[b,i,e] {aggr, h}[b,i,k].
__global__ void __launch_bounds__(kGnBlock) fignn_wgrad_field_kernel(const float* __restrict__ ws,
                                                                     const float* __restrict__ h, int64_t B, int F, int E,
                                                                     float* __restrict__ part) {
  extern __shared__ float4 sv4[];                                  // [sample][da | aggr | dh_out | h][E]
  float* sv = reinterpret_cast<float*>(sv4);
  const int i = blockIdx.x, E4 = E / 4, EE = E * E;
  const int64_t b0 = (int64_t)blockIdx.y * kGnFieldChunk;
  const int nb = B - b0 < kGnFieldChunk ? (int)(B - b0) : kGnFieldChunk;
  for (int t = threadIdx.x; t < nb * 4 * E4; t += kGnBlock) {
    const int sidx = t / (4 * E4), rem = t - sidx * 4 * E4, v = rem / E4, c = rem - v * E4;
    const int64_t row = (b0 + sidx) * F + i;
    const float* src = v == 3 ? h + row * E
                              : ws + (row * kWsVecs + (v == 0 ? kWsDa : v == 1 ? kWsAggr : kWsDho)) * E;
    sv4[t] = reinterpret_cast<const float4*>(src)[c];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * EE; t += kGnBlock) {
    const int m = t / EE, r = t - m * EE, e = r / E, k = r - e * E;
    const float* pe = sv + (2 * m) * E + e;
    const float* pk = sv + (2 * m + 1) * E + k;
    float acc = 0.f;
    for (int sidx = 0; sidx < nb; ++sidx) acc = fmaf(pe[sidx * 4 * E], pk[sidx * 4 * E], acc);
    part[(((int64_t)blockIdx.y * 2 + m) * F + i) * EE + r] = acc;
  }
}

// Chunk c of 64 (sample, field) rows: part[c] = [dW_ih 3E*E | dW_hh 3E*E | db_ih 3E | db_hh 3E | dbias_p E].
__global__ void __launch_bounds__(kGnBlock) fignn_wgrad_gru_kernel(const float* __restrict__ ws,
                                                                   const float* __restrict__ h, int64_t R, int E,
                                                                   float* __restrict__ part) {
  extern __shared__ float4 sv4[];                                  // [row][a | h | dr | dz | dn | dhn | da][E]
  float* sv = reinterpret_cast<float*>(sv4);
  const int E4 = E / 4, EE = E * E, RS = 7 * E;
  const int64_t r0 = (int64_t)blockIdx.x * kGnGruChunk;
  const int nr = R - r0 < kGnGruChunk ? (int)(R - r0) : kGnGruChunk;
  for (int t = threadIdx.x; t < nr * 7 * E4; t += kGnBlock) {
    const int ridx = t / (7 * E4), rem = t - ridx * 7 * E4, v = rem / E4, c = rem - v * E4;
    const int64_t row = r0 + ridx;
    const int wv = v == 0 ? kWsA : v == 6 ? kWsDa : v + 2;        // v = 2..5 -> dr, dz, dn, dhn
    const float* src = v == 1 ? h + row * E : ws + (row * kWsVecs + wv) * E;
    sv4[t] = reinterpret_cast<const float4*>(src)[c];
  }
  __syncthreads();
  const int n = 6 * EE + 7 * E;
  float* pr = part + (int64_t)blockIdx.x * n;
  for (int t = threadIdx.x; t < n; t += kGnBlock) {
    float acc = 0.f;
    if (t < 6 * EE) {
      const int hh = t >= 3 * EE, u = t - hh * 3 * EE, q = u / EE, r = u - q * EE, e = r / E, k = r - e * E;
      const float* pe = sv + ((hh && q == 2) ? 5 : 2 + q) * E + e;
      const float* pk = sv + hh * E + k;
      for (int ridx = 0; ridx < nr; ++ridx) acc = fmaf(pe[ridx * RS], pk[ridx * RS], acc);
    } else {
      const int u = t - 6 * EE;
      int v, e;
      if (u < 3 * E) {
        v = 2 + u / E;
        e = u % E;
      } else if (u < 6 * E) {
        const int q = (u - 3 * E) / E;
        v = q == 2 ? 5 : 2 + q;
        e = u % E;
      } else {
        v = 6;
        e = u - 6 * E;
      }
      const float* pe = sv + v * E + e;
      for (int ridx = 0; ridx < nr; ++ridx) acc += pe[ridx * RS];
    }
    pr[t] = acc;
  }
}

// Column c of the partial rows goes to its segment's destination: columns [0, e0) -> d0, [e0, e1) -> d1, ...; bit k
// of `accmask`: segment k is added to, not overwritten.  A workgroup takes 32 columns; its 8 row slices each add the
// rows r = slice, slice + 8, ... in order (fp64), and the slices are added in order: the same sum on every run.
constexpr int kGnSumCols = 32, kGnSumSlices = kGnBlock / kGnSumCols;
__global__ void __launch_bounds__(kGnBlock) fignn_sum_kernel(const float* __restrict__ part, int64_t G, int ld,
                                                             float* d0, int e0, float* d1, int e1, float* d2, int e2,
                                                             float* d3, int e3, float* d4, int accmask) {
  __shared__ double sh[kGnSumSlices][kGnSumCols];
  const int col = threadIdx.x % kGnSumCols, slice = threadIdx.x / kGnSumCols;
  const int c = blockIdx.x * kGnSumCols + col;
  double a0 = 0.0, a1 = 0.0;
  if (c < ld) {
    const float* src = part + c;
    int64_t r = slice;
    for (; r + kGnSumSlices < G; r += 2 * kGnSumSlices) {
      a0 += src[r * ld];
      a1 += src[(r + kGnSumSlices) * ld];
    }
    if (r < G) a0 += src[r * ld];
  }
  sh[slice][col] = a0 + a1;
  __syncthreads();
  if (slice != 0 || c >= ld) return;
  double t = sh[0][col];
#pragma unroll
  for (int k = 1; k < kGnSumSlices; ++k) t += sh[k][col];
  const float s = (float)t;
  float* p;
  int k;
  if (c < e0) { p = d0 + c; k = 0; }
  else if (c < e1) { p = d1 + (c - e0); k = 1; }
  else if (c < e2) { p = d2 + (c - e1); k = 2; }
  else if (c < e3) { p = d3 + (c - e2); k = 3; }
  else { p = d4 + (c - e3); k = 4; }
  *p = ((accmask >> k) & 1) ? *p + s : s;
}

// ------------------------------------------------------------------------------------------------ prediction
__global__ void __launch_bounds__(kGnBlock) fignn_pred_fwd_kernel(const float* __restrict__ score,
                                                                  const float* __restrict__ z2, int64_t B, int F,
                                                                  float* __restrict__ logits) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (int64_t b = (int64_t)blockIdx.x * kGnWaves + wave; b < B; b += (int64_t)gridDim.x * kGnWaves) {
    const float v = lane < F ? gn_sigmoid(z2[b * F + lane]) * score[b * F + lane] : 0.f;
    const float s = group_sum<kWave>(v);
    if (lane == 0) logits[b] = s;
  }
}

__global__ void __launch_bounds__(kGnBlock) fignn_pred_bwd_kernel(const float* __restrict__ gl,
                                                                  const float* __restrict__ score,
                                                                  const float* __restrict__ z2, int64_t total, int F,
                                                                  float* __restrict__ dscore, float* __restrict__ dz2) {
  for (int64_t t = (int64_t)blockIdx.x * kGnBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kGnBlock) {
    const float gv = gl[t / F], w = gn_sigmoid(z2[t]);
    dscore[t] = gv * w;
    dz2[t] = gv * score[t] * w * (1.f - w);
  }
}

// ------------------------------------------------------------------------------------------------ host
static hipError_t gn_raise_lds_limit() {
  static const hipError_t done =
      allow_dynamic_lds(kGnLdsLimit, &fignn_layer_fwd_kernel<true>, &fignn_layer_fwd_kernel<false>,
                        &fignn_layer_bwd_kernel<true>, &fignn_layer_bwd_kernel<false>);
  return done;
}

static int gn_shape_check(const char* what, int64_t B, int F, int E) {
  MAPX_REQUIRE(B >= 0 && B < (1LL << 31), "%s: bad batch size", what);
  MAPX_REQUIRE(F >= 2 && F <= kGnMaxF, "%s: 2..%d fields (num_fields=%d)", what, kGnMaxF, F);
  MAPX_REQUIRE(E >= 4 && E % 4 == 0 && E <= kGnMaxE, "%s: embed_size %% 4 == 0, <= %d (embed_size=%d)", what, kGnMaxE, E);
  return MAPX_OK;
}

static size_t gn_layer_lds(int F, int E, int nbuf, bool* staged) {
  const size_t fixed = gn_gru_floats(E) + gn_sample_floats(F, E, nbuf);
  *staged = (fixed + gn_weight_floats(F, E)) * sizeof(float) <= kGnStageLimit;
  return (fixed + (*staged ? gn_weight_floats(F, E) : 0)) * sizeof(float);
}

static int gn_tile(int64_t B) {
  const int64_t s = ceil_div(B, 512);
  return (int)(s < 1 ? 1 : s > kGnMaxTile ? kGnMaxTile : s);
}

static int gn_wave_grid(int64_t B) {
  const int64_t g = ceil_div(B, kGnWaves);
  return (int)(g < 1 ? 1 : g > 512 ? 512 : g);
}

}  // namespace mapx

extern "C" int mapx_fignn_weights_staged(int F, int E, int backward) {
  using namespace mapx;
  bool staged = false;
  if (F < 2 || F > kGnMaxF || E < 4 || E % 4 || E > kGnMaxE) return -1;
  gn_layer_lds(F, E, backward ? kGnBwdBufs : kGnFwdBufs, &staged);
  return staged ? 1 : 0;
}

extern "C" int mapx_fignn_graph_fwd(const float* x, const float* w_attn, int64_t B, int F, int E, float* g, float* s,
                                    float* d, hipStream_t stream) {
  using namespace mapx;
  if (int rc = gn_shape_check("fignn_graph_fwd", B, F, E)) return rc;
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(x && w_attn && g && s && d, "fignn_graph_fwd: null pointer");
  const size_t lds = (size_t)kGnWaves * F * (E + 4) * sizeof(float);
  hipLaunchKernelGGL(fignn_graph_fwd_kernel, dim3((unsigned)gn_wave_grid(B)), dim3(kGnBlock), lds, stream, x, w_attn, B,
                     F, E, g, s, d);
  return check_launch("fignn_graph_fwd");
}

extern "C" int mapx_fignn_graph_bwd_groups(int64_t B) { return mapx::gn_wave_grid(B) * mapx::kGnWaves; }

extern "C" int mapx_fignn_graph_bwd(const float* dg, const float* g, const float* s, const float* d, const float* x,
                                    const float* w_attn, const float* dx_base, const float* dx_add_opt, int64_t B, int F,
                                    int E, float* dx, float* part, float* dw_attn, hipStream_t stream) {
  using namespace mapx;
  if (int rc = gn_shape_check("fignn_graph_bwd", B, F, E)) return rc;
  MAPX_REQUIRE(B >= 1, "fignn_graph_bwd: empty batch");
  MAPX_REQUIRE(dg && g && s && d && x && w_attn && dx_base && dx && part && dw_attn, "fignn_graph_bwd: null pointer");
  const int grid = gn_wave_grid(B);
  const size_t lds = (size_t)kGnWaves * (F * (E + 4) + 2 * kWave) * sizeof(float);
  hipLaunchKernelGGL(fignn_graph_bwd_kernel, dim3((unsigned)grid), dim3(kGnBlock), lds, stream, dg, g, s, d, x, w_attn,
                     dx_base, dx_add_opt, B, F, E, dx, part);
  if (int rc = check_launch("fignn_graph_bwd")) return rc;
  const int ld = 2 * E;
  hipLaunchKernelGGL(fignn_sum_kernel, dim3((unsigned)ceil_div(ld, kGnSumCols)), dim3(kGnBlock), 0, stream, part,
                     (int64_t)grid * kGnWaves, ld, dw_attn, ld, (float*)nullptr, ld, (float*)nullptr, ld,
                     (float*)nullptr, ld, (float*)nullptr, 0);
  return check_launch("fignn_graph_bwd_sum");
}

extern "C" int mapx_fignn_layer_fwd(const float* h, const float* g, const float* x_res_opt, const float* w_in,
                                    const float* w_out, const float* bias_p, const float* w_ih, const float* w_hh,
                                    const float* b_ih, const float* b_hh, int64_t B, int F, int E, float* h_next,
                                    hipStream_t stream) {
  using namespace mapx;
  if (int rc = gn_shape_check("fignn_layer_fwd", B, F, E)) return rc;
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(h && g && w_in && w_out && bias_p && w_ih && w_hh && b_ih && b_hh && h_next,
               "fignn_layer_fwd: null pointer");
  bool staged;
  const size_t lds = gn_layer_lds(F, E, kGnFwdBufs, &staged);
  MAPX_REQUIRE(lds <= kGnLdsLimit, "fignn_layer_fwd: num_fields=%d, embed_size=%d take %zu bytes of LDS, above %zu", F,
               E, lds, kGnLdsLimit);
  MAPX_HIP(gn_raise_lds_limit());
  const int S = gn_tile(B);
  const dim3 grid((unsigned)ceil_div(B, S));
  if (staged)
    hipLaunchKernelGGL(fignn_layer_fwd_kernel<true>, grid, dim3(kGnBlock), lds, stream, h, g, x_res_opt, w_in, w_out,
                       bias_p, w_ih, w_hh, b_ih, b_hh, B, S, F, E, h_next);
  else
    hipLaunchKernelGGL(fignn_layer_fwd_kernel<false>, grid, dim3(kGnBlock), lds, stream, h, g, x_res_opt, w_in, w_out,
                       bias_p, w_ih, w_hh, b_ih, b_hh, B, S, F, E, h_next);
  return check_launch("fignn_layer_fwd");
}

extern "C" int mapx_fignn_layer_bwd(const float* dh_next, const float* h, const float* g, const float* w_in,
                                    const float* w_out, const float* bias_p, const float* w_ih, const float* w_hh,
                                    const float* b_ih, const float* b_hh, int64_t B, int F, int E, float* dh, float* dg,
                                    int dg_init, float* dx_acc_opt, int dx_init, float* ws, hipStream_t stream) {
  using namespace mapx;
  if (int rc = gn_shape_check("fignn_layer_bwd", B, F, E)) return rc;
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(dh_next && h && g && w_in && w_out && bias_p && w_ih && w_hh && b_ih && b_hh && dh && dg && ws,
               "fignn_layer_bwd: null pointer");
  MAPX_REQUIRE(dh != dh_next, "fignn_layer_bwd: dh and dh_next must be different buffers");
  bool staged;
  const size_t lds = gn_layer_lds(F, E, kGnBwdBufs, &staged);
  MAPX_REQUIRE(lds <= kGnLdsLimit, "fignn_layer_bwd: num_fields=%d, embed_size=%d take %zu bytes of LDS, above %zu", F,
               E, lds, kGnLdsLimit);
  MAPX_HIP(gn_raise_lds_limit());
  const int S = gn_tile(B);
  const dim3 grid((unsigned)ceil_div(B, S));
  if (staged)
    hipLaunchKernelGGL(fignn_layer_bwd_kernel<true>, grid, dim3(kGnBlock), lds, stream, dh_next, h, g, w_in, w_out,
                       bias_p, w_ih, w_hh, b_ih, b_hh, B, S, F, E, dh, dg, dg_init, dx_acc_opt, dx_init, ws);
  else
    hipLaunchKernelGGL(fignn_layer_bwd_kernel<false>, grid, dim3(kGnBlock), lds, stream, dh_next, h, g, w_in, w_out,
                       bias_p, w_ih, w_hh, b_ih, b_hh, B, S, F, E, dh, dg, dg_init, dx_acc_opt, dx_init, ws);
  return check_launch("fignn_layer_bwd");
}

extern "C" int mapx_fignn_wgrad_groups(int64_t B, int F, int gru) {
  using namespace mapx;
  return (int)(gru ? ceil_div(B * F, kGnGruChunk) : ceil_div(B, kGnFieldChunk));
}

extern "C" int mapx_fignn_layer_wgrad(const float* ws, const float* h, int64_t B, int F, int E, float* part_field,
                                      float* part_gru, float* dw_in, float* dw_out, float* dbias_p, float* dw_ih,
                                      float* dw_hh, float* db_ih, float* db_hh, int add_layer, int add_gru,
                                      hipStream_t stream) {
  using namespace mapx;
  if (int rc = gn_shape_check("fignn_layer_wgrad", B, F, E)) return rc;
  MAPX_REQUIRE(B >= 1, "fignn_layer_wgrad: empty batch");
  MAPX_REQUIRE(ws && h && part_field && part_gru && dw_in && dw_out && dbias_p && dw_ih && dw_hh && db_ih && db_hh,
               "fignn_layer_wgrad: null pointer");
  const int Gf = mapx_fignn_wgrad_groups(B, F, 0), Gg = mapx_fignn_wgrad_groups(B, F, 1);
  const int EE = E * E, FEE = F * EE;
  hipLaunchKernelGGL(fignn_wgrad_field_kernel, dim3((unsigned)F, (unsigned)Gf), dim3(kGnBlock),
                     (size_t)kGnFieldChunk * 4 * E * sizeof(float), stream, ws, h, B, F, E, part_field);
  if (int rc = check_launch("fignn_wgrad_field")) return rc;
  hipLaunchKernelGGL(fignn_wgrad_gru_kernel, dim3((unsigned)Gg), dim3(kGnBlock),
                     (size_t)kGnGruChunk * 7 * E * sizeof(float), stream, ws, h, B * F, E, part_gru);
  if (int rc = check_launch("fignn_wgrad_gru")) return rc;
  const int lm = add_layer ? 1 : 0, gm = add_gru ? 1 : 0;
  hipLaunchKernelGGL(fignn_sum_kernel, dim3((unsigned)ceil_div(2 * FEE, kGnSumCols)), dim3(kGnBlock), 0, stream, part_field,
                     (int64_t)Gf, 2 * FEE, dw_in, FEE, dw_out, 2 * FEE, (float*)nullptr, 2 * FEE, (float*)nullptr,
                     2 * FEE, (float*)nullptr, lm * 3);
  if (int rc = check_launch("fignn_wgrad_field_sum")) return rc;
  const int ld = 6 * EE + 7 * E;
  hipLaunchKernelGGL(fignn_sum_kernel, dim3((unsigned)ceil_div(ld, kGnSumCols)), dim3(kGnBlock), 0, stream, part_gru,
                     (int64_t)Gg, ld, dw_ih, 3 * EE, dw_hh, 6 * EE, db_ih, 6 * EE + 3 * E, db_hh, 6 * EE + 6 * E,
                     dbias_p, gm * 15 + lm * 16);
  return check_launch("fignn_wgrad_gru_sum");
}

extern "C" int mapx_fignn_pred_fwd(const float* score, const float* z2, int64_t B, int F, float* logits,
                                   hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 0 && B < (1LL << 31) && F >= 1 && F <= kGnMaxF, "fignn_pred_fwd: 1..%d fields (num_fields=%d)",
               kGnMaxF, F);
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(score && z2 && logits, "fignn_pred_fwd: null pointer");
  hipLaunchKernelGGL(fignn_pred_fwd_kernel, dim3((unsigned)gn_wave_grid(B)), dim3(kGnBlock), 0, stream, score, z2, B, F,
                     logits);
  return check_launch("fignn_pred_fwd");
}

extern "C" int mapx_fignn_pred_bwd(const float* g_logits, const float* score, const float* z2, int64_t B, int F,
                                   float* dscore, float* dz2, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(B >= 0 && B < (1LL << 31) && F >= 1 && F <= kGnMaxF, "fignn_pred_bwd: 1..%d fields (num_fields=%d)",
               kGnMaxF, F);
  if (B == 0) return MAPX_OK;
  MAPX_REQUIRE(g_logits && score && z2 && dscore && dz2, "fignn_pred_bwd: null pointer");
  hipLaunchKernelGGL(fignn_pred_bwd_kernel, dim3((unsigned)grid_for(B * F, kGnBlock)), dim3(kGnBlock), 0, stream,
                     g_logits, score, z2, B * F, F, dscore, dz2);
  return check_launch("fignn_pred_bwd");
}
