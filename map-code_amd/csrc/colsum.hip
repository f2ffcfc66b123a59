// The small kernels around the dense products, fp32 and bf16 compute mode: column sums (bias gradients) alone and
// fused with the elementwise backward step of a ReLU or cross layer, the deferred slab / partial-row sums, the ReLU
// mask and the fp32 <-> bf16 casts.  The products themselves are gemm_x3.hip / gemm_h2*.hip (fp32) and gemm_bf16.hip.
//
// A column sum is two stages: stage 1 leaves kColChunks partial rows [kColChunks][N] in the caller's workspace (one
// row chunk of the matrix each, lanes' sums met in LDS in a fixed order), stage 2 adds them in chunk order — at once,
// or (out == NULL) later with the step's other partial sums in one mapx_sum_tasks launch.  The element types share
// the chunk count, the workspace, stage 2 and the entries' tail; stage 1 is per type (fp32: float4 lanes, 32 or 64
// per block, and the magnitude record; bf16: 8-column or column-pair lanes), because its geometry is the order of adds.
#include "../../include/mapx_hip.h"
#include "amax.h"
#include "common.h"

namespace mapx {

// Deferred slab sums: dst[i] = sum_s src[s*stride + i] for up to kMaxSumTasks independent
// tasks in ONE launch (split-K slabs of the weight-gradient GEMMs and the row-chunk partials
// of the bias-gradient column sums of a whole backward pass; 14 tiny launches -> 1).
constexpr int kMaxSumTasks = 32;
struct SumTasks {
  mapx_sum_task t[kMaxSumTasks];
};
__global__ void __launch_bounds__(256) sum_tasks_kernel(SumTasks tasks) {
  const mapx_sum_task tk = tasks.t[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tk.n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    int s = 0;
    // The kernel is a latency chain (a column has one thread, a task a few blocks): 32 loads in flight per
    // round trip — 128 row-chunk partials of a bias gradient are 4 round trips, not 16 — added in slab order.
    for (; s + 32 <= tk.nsplit; s += 32) {
      float x[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) x[u] = tk.src[(s + u) * tk.stride + i];
#pragma unroll
      for (int u = 0; u < 32; ++u) v += x[u];
    }
    for (; s + 8 <= tk.nsplit; s += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = tk.src[(s + u) * tk.stride + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += x[u];
    }
    for (; s < tk.nsplit; ++s) v += tk.src[s * tk.stride + i];
    tk.dst[i] = v;
  }
}

// (gemm.hip's batched weight gradient sums its problems' slabs through this too)
void sum_tasks_launch(const mapx_sum_task* tasks, int ntasks, hipStream_t stream) {
  SumTasks t;
  memset(&t, 0, sizeof(t));
  for (int i = 0; i < ntasks; ++i) t.t[i] = tasks[i];
  hipLaunchKernelGGL(sum_tasks_kernel, dim3(96, ntasks), dim3(256), 0, stream, t);
}

// column sums of X [M,N] (bias gradients): stage 1 = kColChunks row chunks -> partial[kColChunks][N]
constexpr int kColChunks = 128;
__global__ void __launch_bounds__(256) colsum_stage1_kernel(const float* __restrict__ x, int64_t ld,
                                                            int M, int N, float* __restrict__ part) {
  // block = 64 columns x 4 row lanes
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const int rows_per = (M + kColChunks - 1) / kColChunks;
  const int r0 = blockIdx.y * rows_per;
  const int r1 = (r0 + rows_per < M) ? r0 + rows_per : M;
  float v = 0.f;
  if (c < N) {
#pragma unroll 8                 // eight loads in flight, added in the same order (a tall narrow matrix — xDeepFM's
    for (int r = r0 + rl; r < r1; r += 4) v += x[(int64_t)r * ld + c];   // [65536, 50] — is one block per chunk: 51 us)
  }
  __shared__ float s[4][64];
  s[rl][threadIdx.x & 63] = v;
  __syncthreads();
  if (rl == 0 && c < N)
    part[(int64_t)blockIdx.y * N + c] = s[0][threadIdx.x] + s[1][threadIdx.x] + s[2][threadIdx.x] +
                                        s[3][threadIdx.x];
}
__global__ void __launch_bounds__(256) colsum_stage2_kernel(const float* __restrict__ part, int N,
                                                            float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float v = 0.f;
  for (int i = 0; i < kColChunks; ++i) v += part[(int64_t)i * N + c];
  out[c] = v;
}

// CrossNetV2 backward, elementwise part of one layer (layers.py:200 differentiated):
//   t = g * x0 (feeds the dXi / dW GEMMs and db),  dx0 (+)= g * u
__global__ void __launch_bounds__(256) cross_bwd_pre_kernel(const float* __restrict__ g,
                                                            const float* __restrict__ x0,
                                                            const float* __restrict__ u, int64_t n4,
                                                            float* __restrict__ t,
                                                            float* __restrict__ dx0, int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    const float4 xv = reinterpret_cast<const float4*>(x0)[i];
    const float4 uv = reinterpret_cast<const float4*>(u)[i];
    reinterpret_cast<float4*>(t)[i] = make_float4(gv.x * xv.x, gv.y * xv.y, gv.z * xv.z, gv.w * xv.w);
    float4 d = make_float4(gv.x * uv.x, gv.y * uv.y, gv.z * uv.z, gv.w * uv.w);
    if (accumulate) {
      const float4 o = reinterpret_cast<const float4*>(dx0)[i];
      d.x += o.x; d.y += o.y; d.z += o.z; d.w += o.w;
    }
    reinterpret_cast<float4*>(dx0)[i] = d;
  }
}

// Elementwise backward steps fused with the bias-gradient column sum (one pass over the
// data instead of elementwise kernel + colsum stage 1):
//   OP 0 (ReLU layer):   dz = y > 0 ? dy : 0                      db = colsum(dz)
//   OP 1 (cross layer):  t = g * x0 ; dx0 (+)= g * u (+ g)        db = colsum(t)
//                        accumulate bit 0: add to the dx0 already there; bit 1: also add g
// Block = CL column lanes (x float4) x 256 / CL row lanes over one of kColChunks row chunks; stage 2 adds the
// chunks.  CL = 64 or 32, whichever wastes fewer lanes on the last column block (N = 368: 92 float4 columns
// are 2 blocks of 64 with 28 % of the lanes idle, or 3 blocks of 32 with 4 %).
template <int OP, int CL>
__global__ void __launch_bounds__(256) ew_colsum_kernel(const float* __restrict__ a, int64_t lda,
                                                        const float* __restrict__ b, int64_t ldb,
                                                        const float* __restrict__ c, int M, int N,
                                                        float* __restrict__ o1, float* __restrict__ o2,
                                                        int accumulate, float* __restrict__ part,
                                                        amax_rec* __restrict__ amax_o1, const int32_t* __restrict__ epoch) {
  // CL lanes x float4 columns per block row; RL row lanes; N % 4 == 0, lda % 4 == 0 (host-checked)
  constexpr int RL = 256 / CL;
  const int cl = threadIdx.x % CL;
  const int col = (blockIdx.x * CL + cl) * 4;
  const int rl = threadIdx.x / CL;
  const int rows_per = (M + kColChunks - 1) / kColChunks;
  const int r0 = blockIdx.y * rows_per;
  const int r1 = (r0 + rows_per < M) ? r0 + rows_per : M;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  uint32_t amx = 0;                     // max |o1| (dz or t) for the products that read it next (amax.h)
  if (col < N) {
#pragma unroll 4
    for (int r = r0 + rl; r < r1; r += RL) {
      const int64_t i = ((int64_t)r * N + col) >> 2;
      const float4 av = reinterpret_cast<const float4*>(a)[((int64_t)r * lda + col) >> 2];   // a may be a column slice
      const float4 bv = reinterpret_cast<const float4*>(b)[((int64_t)r * ldb + col) >> 2];
      if (OP == 0) {
        const float4 dz = make_float4(bv.x > 0.f ? av.x : 0.f, bv.y > 0.f ? av.y : 0.f,
                                      bv.z > 0.f ? av.z : 0.f, bv.w > 0.f ? av.w : 0.f);
        reinterpret_cast<float4*>(o1)[i] = dz;
        amx = amax4(amx, dz.x, dz.y, dz.z, dz.w);
        v.x += dz.x; v.y += dz.y; v.z += dz.z; v.w += dz.w;
      } else {
        const float4 cv = reinterpret_cast<const float4*>(c)[i];
        const float4 t = make_float4(av.x * bv.x, av.y * bv.y, av.z * bv.z, av.w * bv.w);
        float4 d = make_float4(av.x * cv.x, av.y * cv.y, av.z * cv.z, av.w * cv.w);
        if (accumulate & 1) {
          const float4 o = reinterpret_cast<const float4*>(o2)[i];
          d.x += o.x; d.y += o.y; d.z += o.z; d.w += o.w;
        }
        if (accumulate & 2) {   // first cross layer: Xi IS X0, its gradient g joins the X0 total
          d.x += av.x; d.y += av.y; d.z += av.z; d.w += av.w;
        }
        reinterpret_cast<float4*>(o1)[i] = t;
        amx = amax4(amx, t.x, t.y, t.z, t.w);
        reinterpret_cast<float4*>(o2)[i] = d;
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
      }
    }
  }
  if (amax_o1) amax_publish_block(amax_o1, amx, epoch);
  __shared__ float4 s[RL][CL];
  s[rl][cl] = v;
  __syncthreads();
  if (rl == 0 && col < N) {
    float4 t = s[0][cl];
#pragma unroll
    for (int k = 1; k < RL; ++k) {       // fixed order: bit-reproducible
      const float4 q = s[k][cl];
      t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
    }
    *reinterpret_cast<float4*>(part + (int64_t)blockIdx.y * N + col) = t;
  }
}

// 32 instead of 64 column lanes per block when that leaves fewer lanes of the last column block idle
static inline bool ew_narrow_lanes(int N) {
  const int c4 = (N + 3) / 4;
  return ((c4 + 31) / 32) * 32 < ((c4 + 63) / 64) * 64;
}

// The bf16 path's stage 1 (activations bf16, sums fp32), the operations above and the plain sum:
//   OP 0 (ReLU layer):   dz = y > 0 ? dy : 0                      db = colsum(dz)
//   OP 1 (cross layer):  t = g * x0 ; dx0 (+)= g * u (+ g)        db = colsum(t)     (dx0 kept in fp32)
//   OP 2 (plain):        nothing written                          db = colsum(a)
// Block = 64 column lanes x 4 row lanes over one of kColChunks row chunks.  Scalar columns: any N, any leading
// dimension.
template <int OP>
__global__ void __launch_bounds__(256) ew_colsum_h_kernel(const bf16_t* __restrict__ a, int64_t lda,
                                                          const bf16_t* __restrict__ b, int64_t ldb,
                                                          const bf16_t* __restrict__ c, int64_t ldc, int M, int N,
                                                          bf16_t* __restrict__ o1, float* __restrict__ o2,
                                                          int accumulate, float* __restrict__ part) {
  const int col = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2;      // 2 columns per lane (one dword of bf16)
  const int rl = threadIdx.x >> 6;
  const int rows_per = (M + kColChunks - 1) / kColChunks;
  const int r0 = blockIdx.y * rows_per;
  const int r1 = (r0 + rows_per < M) ? r0 + rows_per : M;
  float v0 = 0.f, v1 = 0.f;
  const bool in0 = col < N, in1 = col + 1 < N;
  if (in0) {
    for (int r = r0 + rl; r < r1; r += 4) {
      const float a0 = (float)a[(int64_t)r * lda + col], a1 = in1 ? (float)a[(int64_t)r * lda + col + 1] : 0.f;
      if (OP == 2) {
        v0 += a0; v1 += a1;
      } else if (OP == 0) {
        const float y0 = (float)b[(int64_t)r * ldb + col], y1 = in1 ? (float)b[(int64_t)r * ldb + col + 1] : 0.f;
        const float d0 = y0 > 0.f ? a0 : 0.f, d1 = y1 > 0.f ? a1 : 0.f;
        o1[(int64_t)r * N + col] = (bf16_t)d0;
        if (in1) o1[(int64_t)r * N + col + 1] = (bf16_t)d1;
        v0 += d0; v1 += d1;
      } else {
        const float x0 = (float)b[(int64_t)r * ldb + col], x1 = in1 ? (float)b[(int64_t)r * ldb + col + 1] : 0.f;
        const float u0 = (float)c[(int64_t)r * ldc + col], u1 = in1 ? (float)c[(int64_t)r * ldc + col + 1] : 0.f;
        const bf16_t t0 = (bf16_t)(a0 * x0), t1 = (bf16_t)(a1 * x1);
        float d0 = a0 * u0, d1 = a1 * u1;
        if (accumulate & 1) { d0 += o2[(int64_t)r * N + col]; if (in1) d1 += o2[(int64_t)r * N + col + 1]; }
        if (accumulate & 2) { d0 += a0; d1 += a1; }
        o1[(int64_t)r * N + col] = t0;
        o2[(int64_t)r * N + col] = d0;
        if (in1) { o1[(int64_t)r * N + col + 1] = t1; o2[(int64_t)r * N + col + 1] = d1; }
        v0 += (float)t0; v1 += (float)t1;        // db is the column sum of what the dW GEMM reads
      }
    }
  }
  __shared__ float s[4][128];
  s[rl][2 * (threadIdx.x & 63)] = v0;
  s[rl][2 * (threadIdx.x & 63) + 1] = v1;
  __syncthreads();
  if (rl == 0 && in0) {
    const int k = 2 * threadIdx.x;
    part[(int64_t)blockIdx.y * N + col] = s[0][k] + s[1][k] + s[2][k] + s[3][k];
    if (in1) part[(int64_t)blockIdx.y * N + col + 1] = s[0][k + 1] + s[1][k + 1] + s[2][k + 1] + s[3][k + 1];
  }
}
// The same three operations, 8 columns (one 16-byte bf16 chunk) per lane: N % 8 == 0, leading
// dimensions % 8 == 0, 16-byte aligned bases (the trunk's widths 368 / 400 / 624 / 1000 / 736 all are).
// (The chunks stay bf16 vectors: dz is a select between bf16 values, and t is needed both as stored and widened.)
template <int OP>
__global__ void __launch_bounds__(256) ew_colsum_h8_kernel(const bf16_t* __restrict__ a, int64_t lda,
                                                           const bf16_t* __restrict__ b, int64_t ldb,
                                                           const bf16_t* __restrict__ c, int64_t ldc, int M, int N,
                                                           bf16_t* __restrict__ o1, float* __restrict__ o2,
                                                           int accumulate, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + lane) * 8;
  const int rows_per = (M + kColChunks - 1) / kColChunks;
  const int r0 = blockIdx.y * rows_per;
  const int r1 = (r0 + rows_per < M) ? r0 + rows_per : M;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.f;
  if (col < N) {
#pragma unroll 2
    for (int r = r0 + rl; r < r1; r += 4) {
      const bf16x8_t av = *reinterpret_cast<const bf16x8_t*>(a + (int64_t)r * lda + col);
      if (OP == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += (float)av[e];
      } else if (OP == 0) {
        const bf16x8_t yv = *reinterpret_cast<const bf16x8_t*>(b + (int64_t)r * ldb + col);
        bf16x8_t d;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          d[e] = (float)yv[e] > 0.f ? av[e] : (bf16_t)0.f;
          v[e] += (float)d[e];
        }
        *reinterpret_cast<bf16x8_t*>(o1 + (int64_t)r * N + col) = d;
      } else {
        const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(b + (int64_t)r * ldb + col);
        const bf16x8_t uv = *reinterpret_cast<const bf16x8_t*>(c + (int64_t)r * ldc + col);
        float4 d0 = make_float4(0.f, 0.f, 0.f, 0.f), d1 = d0;
        float* dp = o2 + (int64_t)r * N + col;
        if (accumulate & 1) {
          d0 = *reinterpret_cast<const float4*>(dp);
          d1 = *reinterpret_cast<const float4*>(dp + 4);
        }
        float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        bf16x8_t t;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float g = (float)av[e];
          t[e] = (bf16_t)(g * (float)xv[e]);
          d[e] += g * (float)uv[e];
          if (accumulate & 2) d[e] += g;
          v[e] += (float)t[e];
        }
        *reinterpret_cast<bf16x8_t*>(o1 + (int64_t)r * N + col) = t;
        *reinterpret_cast<float4*>(dp) = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<float4*>(dp + 4) = make_float4(d[4], d[5], d[6], d[7]);
      }
    }
  }
  __shared__ float s[4][64][9];          // 9: the 8 values of a lane on distinct banks from its neighbours'
#pragma unroll
  for (int e = 0; e < 8; ++e) s[rl][lane][e] = v[e];
  __syncthreads();
  if (rl == 0 && col < N) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = s[0][lane][e] + s[1][lane][e] + s[2][lane][e] + s[3][lane][e];
    float* dst = part + (int64_t)blockIdx.y * N + col;
    *reinterpret_cast<float4*>(dst) = make_float4(t[0], t[1], t[2], t[3]);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(t[4], t[5], t[6], t[7]);
  }
}

// 8-column lanes when every operand allows 16-byte accesses, scalar column pairs otherwise
template <int OP>
static void launch_ew_colsum_h(const bf16_t* a, int64_t lda, const bf16_t* b, int64_t ldb, const bf16_t* c, int64_t ldc,
                               int M, int N, bf16_t* o1, float* o2, int accumulate, float* part, hipStream_t stream) {
  auto al16 = [](const void* p) { return (uintptr_t)p % 16 == 0; };
  const bool vec = N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && al16(a) && al16(b) && al16(c) &&
                   al16(o1) && al16(o2) && al16(part);
  if (vec)
    hipLaunchKernelGGL(ew_colsum_h8_kernel<OP>, dim3((N + 511) / 512, kColChunks), dim3(256), 0, stream, a, lda, b,
                       ldb, c, ldc, M, N, o1, o2, accumulate, part);
  else
    hipLaunchKernelGGL(ew_colsum_h_kernel<OP>, dim3((N + 127) / 128, kColChunks), dim3(256), 0, stream, a, lda, b,
                       ldb, c, ldc, M, N, o1, o2, accumulate, part);
}

// The partial rows of a column sum over N columns in the caller's workspace, or NULL (error set) when it is too small.
static float* colsum_part(const char* what, void* ws, size_t ws_bytes, int N) {
  if (ws && ws_bytes >= mapx_colsum_workspace_bytes(N)) return static_cast<float*>(ws);
  set_error("%s: workspace too small", what);
  return nullptr;
}

// Every entry's tail: stage 2 now, or (out == NULL) the caller adds the kColChunks partial rows later (mapx_sum_tasks).
static int colsum_finish(const char* what, const float* part, int N, float* out, hipStream_t stream) {
  if (out) hipLaunchKernelGGL(colsum_stage2_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, part, N, out);
  return check_launch(what);
}

// ReLU backward: out = y > 0 ? dy : 0  (y = the layer's activated output)
__global__ void __launch_bounds__(256) relu_mask_kernel(const float* __restrict__ dy,
                                                        const float* __restrict__ y, int64_t n,
                                                        float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = y[i] > 0.f ? dy[i] : 0.f;
}
__global__ void __launch_bounds__(256) relu_mask_h_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y,
                                                          int64_t n, bf16_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (float)y[i] > 0.f ? dy[i] : (bf16_t)0.f;
}

// fp32 <-> bf16 conversion of a flat array (weights shadows outside the optimizer, head gradients)
__global__ void __launch_bounds__(256) cast_f32_bf16_kernel(const float* __restrict__ src, int64_t n,
                                                            bf16_t* __restrict__ dst) {
  const int64_t n8 = n / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = reinterpret_cast<const float4*>(src)[2 * i], b = reinterpret_cast<const float4*>(src)[2 * i + 1];
    bf16x8_t o;      // (written out: through common.h's bf16x8_of the compiler addresses the two loads differently)
    o[0] = (bf16_t)a.x; o[1] = (bf16_t)a.y; o[2] = (bf16_t)a.z; o[3] = (bf16_t)a.w;
    o[4] = (bf16_t)b.x; o[5] = (bf16_t)b.y; o[6] = (bf16_t)b.z; o[7] = (bf16_t)b.w;
    reinterpret_cast<bf16x8_t*>(dst)[i] = o;
  }
  if (blockIdx.x == 0)
    for (int64_t i = n8 * 8 + threadIdx.x; i < n; i += blockDim.x) dst[i] = (bf16_t)src[i];
}
__global__ void __launch_bounds__(256) cast_bf16_f32_kernel(const bf16_t* __restrict__ src, int64_t n,
                                                            float* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = (float)src[i];
}

}  // namespace mapx

extern "C" size_t mapx_colsum_workspace_bytes(int N) {
  return (size_t)mapx::kColChunks * N * sizeof(float);
}
extern "C" size_t mapx_colsum_bf16_workspace_bytes(int N) { return mapx_colsum_workspace_bytes(N); }

extern "C" int mapx_colsum_chunks(void) { return mapx::kColChunks; }

extern "C" int mapx_sum_tasks(const mapx_sum_task* tasks_host, int ntasks, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(ntasks >= 0 && ntasks <= kMaxSumTasks, "sum_tasks: at most %d tasks per call", kMaxSumTasks);
  if (ntasks == 0) return MAPX_OK;
  MAPX_REQUIRE(tasks_host, "sum_tasks: null task list");
  for (int i = 0; i < ntasks; ++i)
    MAPX_REQUIRE(tasks_host[i].dst && tasks_host[i].src && tasks_host[i].nsplit >= 1 && tasks_host[i].n >= 0,
                 "sum_tasks: bad task %d", i);
  sum_tasks_launch(tasks_host, ntasks, stream);
  return check_launch("sum_tasks");
}

extern "C" int mapx_colsum(const float* x, int64_t ld, int M, int N, float* out, void* ws,
                           size_t ws_bytes, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(x && M >= 0 && N > 0, "colsum: bad arguments");
  float* part = colsum_part("colsum", ws, ws_bytes, N);
  if (!part) return MAPX_EWORKSPACE;
  hipLaunchKernelGGL(colsum_stage1_kernel, dim3((N + 63) / 64, kColChunks), dim3(256), 0, stream, x,
                     ld, M, N, part);
  return colsum_finish("colsum", part, N, out, stream);
}

extern "C" int mapx_colsum_bf16(const mapx_bf16* x, int64_t ld, int M, int N, float* out, void* ws, size_t ws_bytes,
                                hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(x && M >= 0 && N > 0 && ld >= N, "colsum_bf16: bad arguments");
  float* part = colsum_part("colsum_bf16", ws, ws_bytes, N);
  if (!part) return MAPX_EWORKSPACE;
  launch_ew_colsum_h<2>(hc(x), ld, hc(x), ld, hc(x), ld, M, N, nullptr, nullptr, 0, part, stream);
  return colsum_finish("colsum_bf16", part, N, out, stream);
}

extern "C" int mapx_relu_mask_colsum(const float* dy, int64_t ld_dy, const float* y, int64_t ld_y, int M, int N,
                                     float* dz, float* db, void* ws, size_t ws_bytes, void* amax_out_opt,
                                     hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(dy && y && dz && M >= 0 && N > 0, "relu_mask_colsum: bad arguments");
  MAPX_REQUIRE(N % 4 == 0 && ld_dy % 4 == 0 && ld_dy >= N && (uintptr_t)dy % 16 == 0 && ld_y % 4 == 0 &&
                   ld_y >= N && (uintptr_t)y % 16 == 0,
               "relu_mask_colsum: N, ld_dy, ld_y %% 4 != 0 or dy / y not 16-byte aligned");
  float* part = colsum_part("relu_mask_colsum", ws, ws_bytes, N);
  if (!part) return MAPX_EWORKSPACE;
  if (ew_narrow_lanes(N))
    hipLaunchKernelGGL((ew_colsum_kernel<0, 32>), dim3((N + 127) / 128, kColChunks), dim3(256), 0, stream, dy, ld_dy, y,
                       ld_y, (const float*)nullptr, M, N, dz, (float*)nullptr, 0, part, static_cast<amax_rec*>(amax_out_opt),
                       amax_epoch_ptr());
  else
    hipLaunchKernelGGL((ew_colsum_kernel<0, 64>), dim3((N + 255) / 256, kColChunks), dim3(256), 0, stream, dy, ld_dy, y,
                       ld_y, (const float*)nullptr, M, N, dz, (float*)nullptr, 0, part, static_cast<amax_rec*>(amax_out_opt),
                       amax_epoch_ptr());
  return colsum_finish("relu_mask_colsum", part, N, db, stream);
}

extern "C" int mapx_relu_mask_colsum_bf16(const mapx_bf16* dy, int64_t ld_dy, const mapx_bf16* y, int64_t ld_y, int M,
                                          int N, mapx_bf16* dz, float* db, void* ws, size_t ws_bytes,
                                          hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(dy && y && dz && M >= 0 && N > 0 && ld_dy >= N && ld_y >= N, "relu_mask_colsum_bf16: bad arguments");
  float* part = colsum_part("relu_mask_colsum_bf16", ws, ws_bytes, N);
  if (!part) return MAPX_EWORKSPACE;
  launch_ew_colsum_h<0>(hc(dy), ld_dy, hc(y), ld_y, hc(y), ld_y, M, N, hm(dz), nullptr, 0, part, stream);
  return colsum_finish("relu_mask_colsum_bf16", part, N, db, stream);
}

extern "C" int mapx_cross_bwd_pre_colsum(const float* g, int64_t ld_g, const float* x0, const float* u, int M, int N,
                                         float* t, float* dx0, int accumulate, float* db, void* ws,
                                         size_t ws_bytes, void* amax_out_opt, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(g && x0 && u && t && dx0 && M >= 0 && N > 0, "cross_bwd_pre_colsum: bad arguments");
  MAPX_REQUIRE(N % 4 == 0 && ld_g % 4 == 0 && ld_g >= N && (uintptr_t)g % 16 == 0,
               "cross_bwd_pre_colsum: N, ld_g %% 4 != 0 or g not 16-byte aligned");
  float* part = colsum_part("cross_bwd_pre_colsum", ws, ws_bytes, N);
  if (!part) return MAPX_EWORKSPACE;
  if (ew_narrow_lanes(N))
    hipLaunchKernelGGL((ew_colsum_kernel<1, 32>), dim3((N + 127) / 128, kColChunks), dim3(256), 0, stream, g, ld_g, x0,
                       (int64_t)N, u, M, N, t, dx0, accumulate, part, static_cast<amax_rec*>(amax_out_opt), amax_epoch_ptr());
  else
    hipLaunchKernelGGL((ew_colsum_kernel<1, 64>), dim3((N + 255) / 256, kColChunks), dim3(256), 0, stream, g, ld_g, x0,
                       (int64_t)N, u, M, N, t, dx0, accumulate, part, static_cast<amax_rec*>(amax_out_opt), amax_epoch_ptr());
  return colsum_finish("cross_bwd_pre_colsum", part, N, db, stream);
}

extern "C" int mapx_cross_bwd_pre_colsum_bf16(const mapx_bf16* g, int64_t ld_g, const mapx_bf16* x0, const mapx_bf16* u,
                                              int M, int N, mapx_bf16* t, float* dx0, int accumulate, float* db,
                                              void* ws, size_t ws_bytes, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(g && x0 && u && t && dx0 && M >= 0 && N > 0 && ld_g >= N, "cross_bwd_pre_colsum_bf16: bad arguments");
  float* part = colsum_part("cross_bwd_pre_colsum_bf16", ws, ws_bytes, N);
  if (!part) return MAPX_EWORKSPACE;
  launch_ew_colsum_h<1>(hc(g), ld_g, hc(x0), (int64_t)N, hc(u), (int64_t)N, M, N, hm(t), dx0, accumulate, part, stream);
  return colsum_finish("cross_bwd_pre_colsum_bf16", part, N, db, stream);
}

extern "C" int mapx_cross_bwd_pre(const float* g, const float* x0, const float* u, int64_t n,
                                  float* t, float* dx0, int accumulate, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(g && x0 && u && t && dx0 && n >= 0 && n % 4 == 0, "cross_bwd_pre: bad arguments");
  if (n == 0) return MAPX_OK;
  hipLaunchKernelGGL(cross_bwd_pre_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, stream, g, x0, u,
                     n / 4, t, dx0, accumulate);
  return check_launch("cross_bwd_pre");
}

extern "C" int mapx_relu_mask(const float* dy, const float* y, int64_t n, float* out,
                              hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(dy && y && out && n >= 0, "relu_mask: bad arguments");
  if (n == 0) return MAPX_OK;
  hipLaunchKernelGGL(relu_mask_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, dy, y, n, out);
  return check_launch("relu_mask");
}

extern "C" int mapx_relu_mask_bf16(const mapx_bf16* dy, const mapx_bf16* y, int64_t n, mapx_bf16* out,
                                   hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(dy && y && out && n >= 0, "relu_mask_bf16: bad arguments");
  if (n == 0) return MAPX_OK;
  hipLaunchKernelGGL(relu_mask_h_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, hc(dy), hc(y), n, hm(out));
  return check_launch("relu_mask_bf16");
}

extern "C" int mapx_cast_f32_bf16(const float* src, int64_t n, mapx_bf16* dst, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 0, "cast_f32_bf16: negative size");
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(src && dst && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, "cast_f32_bf16: null or unaligned pointer");
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(ceil_div(n, 8), 256)), dim3(256), 0, stream, src, n, hm(dst));
  return check_launch("cast_f32_bf16");
}

extern "C" int mapx_cast_bf16_f32(const mapx_bf16* src, int64_t n, float* dst, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 0, "cast_bf16_f32: negative size");
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(src && dst, "cast_bf16_f32: null pointer");
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, hc(src), n, dst);
  return check_launch("cast_bf16_f32");
}
