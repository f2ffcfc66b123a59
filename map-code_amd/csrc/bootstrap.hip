// Poisson bootstrap of the evaluation metrics on the device: R resamples of the rows, and per resample the four
// numbers from which the host forms a weighted AUC and log-loss (mapx/score.py: bootstrap_report).
//
//   weight     replicate r gives unit u the integer weight boot_weight(word r % 4 of
//              Philox(seed, ctr_lo = u, ctr_hi = 'BOOT' << 32 | r / 4)): the number of k with word >= T[k],
//              T[k] = floor(2^32 * P(Poisson(1) <= k)), k = 0..11, so 0..12.  A unit is a 64-bit id, the row number
//              unless the caller passes one per row (rows of one unit share a weight: the cluster bootstrap).  The
//              weight is a function of (seed, unit, r) alone: two models scored on the same rows see the same resample.
//   pos_w[r]   sum of w_i y_i;   neg_w[r]  sum of w_i (1 - y_i)
//   u2[r]      sum over tie runs of p32 of  posW_run * (2 negW_before_run + negW_run): twice the weighted U statistic,
//              metrics.hip's quantity with weights.  AUC_r = u2 / (2 pos_w neg_w).
//   sum_loss[r] sum of w_i * logloss_term(p32_i, y_i) in fp64.
//
// Launches of mapx_bootstrap_metrics:
//   1. boot_prepare_kernel    key = bits of p32 (a NaN logit ranks as p = 1), value = the row number
//   2. rocprim::radix_sort_pairs over 30 bits (stable: the sorted sequence is a function of the input)
//   3. boot_rows_kernel       per sorted row: unit id, flags {positive, last row of its tie run}, the loss term, once
//   4. boot_borders_kernel    the n rows are cut into S = boot_segments(n) segments of boot_segment_rows(n) rows, and
//                             each border moves forward to the next tie-run start, so no run crosses one (an all-equal
//                             input is one long segment and S - 1 empty ones).  S depends on n alone, never on the
//                             device, so every fp64 addition has the same place on every machine.
//   5. boot_replicate_kernel  one wave per (replicate quad, segment) streams the segment 64 rows a step: a lane draws
//                             one Philox for its row's unit and has the weights of four replicates; per replicate one
//                             32-bit wave scan of (posW << 16 | negW) (a step holds at most 64 * 12 of either), carries
//                             in 32 bits (12 * 2^28 < 2^32); one ballot of the run-last flags serves all four; a
//                             run-last lane adds (PP - PP_start) * (NP_start + NP), prefixes inside the segment; a lane
//                             adds its w * term to a sum of its own, step after step
//   6. boot_close_kernel      per replicate, segments in order: u2 = sum A_s + 2 posW_s * (negW of the segments before)
// No atomics at all.  The integers are exact; the fp64 sum of a replicate is: per lane over the steps of a segment in
// order, the 64 lanes by a fixed shuffle tree, the segments in order.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr unsigned kBootProbBits = 30;          // fp32 values in [0, 1] have bit patterns <= 0x3F800000 < 2^30
constexpr uint32_t kBootOneBits = 0x3F800000u;
constexpr int64_t kBootMaxRows = (int64_t)1 << 28;
constexpr int kBootMaxReplicates = 65536;
constexpr int kBootMaxSegments = 256;
constexpr int64_t kBootMinSegmentRows = 384;    // six steps of a wave
constexpr uint64_t kBootCounterHi = 0x424F4F54ull << 32;
constexpr uint8_t kBootPositive = 1, kBootRunLast = 2;

// Nominal rows of a segment and the number of segments: functions of n alone.
__host__ __device__ inline int64_t boot_segment_rows(int64_t n) {
  const int64_t even = ceil_div(ceil_div(n, (int64_t)kBootMaxSegments), (int64_t)kWave) * kWave;
  return even > kBootMinSegmentRows ? even : kBootMinSegmentRows;
}
__host__ __device__ inline int boot_segments(int64_t n) { return (int)ceil_div(n, boot_segment_rows(n)); }

// THE weight of a 32-bit word: Poisson(1) by its cumulative distribution, floor(2^32 * sum_{j <= k} e^-1 / j!).
__device__ inline uint32_t boot_weight(uint32_t word) {
  constexpr uint32_t T[12] = {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u,
                              4294609777u, 4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u};
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) w += word >= T[k] ? 1u : 0u;
  return w;
}

struct BootWeights4 {
  uint32_t a, b, c, d;   // replicates 4 q, 4 q + 1, 4 q + 2, 4 q + 3
};

// THE draw: the weights of one unit in the four replicates of quad q.
__device__ inline BootWeights4 boot_weights4(uint64_t seed, uint64_t unit, uint32_t quad) {
  const Philox4 r = philox4x32_10(seed, unit, kBootCounterHi | quad);
  return BootWeights4{boot_weight(r.x), boot_weight(r.y), boot_weight(r.z), boot_weight(r.w)};
}

// w [R, n]: grid.y = quad, grid.x strides the rows.
__global__ void __launch_bounds__(256) boot_weights_kernel(const int64_t* __restrict__ units, int64_t n, int R,
                                                           uint64_t seed, uint8_t* __restrict__ w) {
  const uint32_t q = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const BootWeights4 d = boot_weights4(seed, units ? (uint64_t)units[i] : (uint64_t)i, q);
    const int64_t r = (int64_t)q * 4;
    if (r + 0 < R) w[(r + 0) * n + i] = (uint8_t)d.a;
    if (r + 1 < R) w[(r + 1) * n + i] = (uint8_t)d.b;
    if (r + 2 < R) w[(r + 2) * n + i] = (uint8_t)d.c;
    if (r + 3 < R) w[(r + 3) * n + i] = (uint8_t)d.d;
  }
}

__global__ void __launch_bounds__(256) boot_prepare_kernel(const float* __restrict__ logits, int64_t n,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ rows) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t bits = __float_as_uint(sigmoid_f32(logits[i]));
    keys[i] = bits > kBootOneBits ? kBootOneBits : bits;   // (a NaN logit ranks as 1, as in slice_metrics.hip)
    rows[i] = (uint32_t)i;
  }
}

// Sorted position j -> what every replicate reads of it.
__global__ void __launch_bounds__(256) boot_rows_kernel(const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ rows,
                                                        const float* __restrict__ labels,
                                                        const int64_t* __restrict__ units, int64_t n,
                                                        uint64_t* __restrict__ unit, uint8_t* __restrict__ flag,
                                                        double* __restrict__ term) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const uint32_t k = keys[j], row = rows[j];
    const bool y = labels[row] > 0.5f;
    const bool run_last = (j == n - 1) || (keys[j + 1] != k);
    unit[j] = units ? (uint64_t)units[row] : (uint64_t)row;
    flag[j] = (uint8_t)((y ? kBootPositive : 0) | (run_last ? kBootRunLast : 0));
    term[j] = logloss_term(__uint_as_float(k), y);
  }
}

// starts[s] = the first tie-run start at or behind s * L, s = 0..S (starts[0] = 0, starts[S] = n): one wave per inner
// border looks for the first run-last row from s * L - 1 on.  Row n - 1 is one, so the search ends inside the array.
__global__ void __launch_bounds__(kWave) boot_borders_kernel(const uint8_t* __restrict__ flag, int64_t n, int64_t L,
                                                             int S, int64_t* __restrict__ starts) {
  const int lane = threadIdx.x, s = blockIdx.x;
  if (s == 0 || s == S) {
    if (lane == 0) starts[s] = s == 0 ? 0 : n;
    return;
  }
  for (int64_t j = (int64_t)s * L - 1; j < n; j += kWave) {
    const int64_t i = j + lane;
    const unsigned long long m = __ballot(i < n && (flag[i] & kBootRunLast));
    if (m) {
      if (lane == 0) starts[s] = j + (__ffsll(m) - 1) + 1;
      return;
    }
  }
}

struct BootPartial {
  unsigned long long a;    // the run terms with prefixes taken inside the segment
  uint32_t pos, neg;       // the segment's posW, negW
  double loss;
};

// Inclusive wave scan of 32-bit words.
__device__ inline uint32_t boot_scan(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t t = __shfl_up(v, off);
    v += lane >= off ? t : 0u;
  }
  return v;
}

// One replicate's share of a step.  v: this lane's scanned (posW << 16 | negW) inside the step.
struct BootRep {
  uint32_t cp = 0, cn = 0;   // posW, negW of the segment's rows before this step
  uint32_t rp = 0, rn = 0;   // the same at the end of the last tie run that has ended
  unsigned long long acc = 0;
  double loss = 0.0;

  __device__ inline void step(uint32_t w, uint32_t f, double t, int lane, bool has_prev, int prev, bool any, int last) {
    loss = fma((double)w, t, loss);
    const uint32_t v = boot_scan((f & kBootPositive) ? w << 16 : w, lane);
    const uint32_t at_prev = __shfl(v, prev), at_last = __shfl(v, last), total = __shfl(v, kWave - 1);
    if (f & kBootRunLast) {
      const uint32_t pp = cp + (v >> 16), np = cn + (v & 0xFFFFu);
      const uint32_t ps = has_prev ? cp + (at_prev >> 16) : rp, ns = has_prev ? cn + (at_prev & 0xFFFFu) : rn;
      acc += (unsigned long long)(pp - ps) * ((unsigned long long)ns + np);
    }
    if (any) {
      rp = cp + (at_last >> 16);
      rn = cn + (at_last & 0xFFFFu);
    }
    cp += total >> 16;
    cn += total & 0xFFFFu;
  }

  // lane 0 holds the result
  __device__ inline BootPartial close() const {
    unsigned long long a = acc;
    double l = loss;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      a += __shfl_down(a, off);
      l += __shfl_down(l, off);
    }
    return BootPartial{a, cp, cn, l};
  }
};

// Four waves a block: quads 4 blockIdx.x + wave of segment blockIdx.y (neighbours read the same rows).
// part [S, 4 Q]: segment-major, so that boot_close_kernel's neighbouring threads read neighbouring partials.
__global__ void __launch_bounds__(256) boot_replicate_kernel(const uint64_t* __restrict__ unit,
                                                             const uint8_t* __restrict__ flag,
                                                             const double* __restrict__ term,
                                                             const int64_t* __restrict__ starts, int Q, uint64_t seed,
                                                             BootPartial* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), s = blockIdx.y;
  if (q >= Q) return;   // (uniform over the wave; the kernel has no barrier)
  const int64_t begin = starts[s], end = starts[s + 1];
  BootRep r0, r1, r2, r3;
  for (int64_t j = begin; j < end; j += kWave) {
    const int64_t i = j + lane;
    const bool live = i < end;
    const uint64_t u = live ? unit[i] : 0;
    const uint32_t f = live ? flag[i] : 0u;
    const double t = live ? term[i] : 0.0;
    BootWeights4 w = boot_weights4(seed, u, (uint32_t)q);
    if (!live) w = BootWeights4{0, 0, 0, 0};
    const unsigned long long m = __ballot((f & kBootRunLast) != 0);
    const unsigned long long below = m & ((1ull << lane) - 1ull);
    const bool has_prev = below != 0, any = m != 0;
    const int prev = has_prev ? 63 - __clzll((long long)below) : 0;
    const int last = any ? 63 - __clzll((long long)m) : 0;
    r0.step(w.a, f, t, lane, has_prev, prev, any, last);
    r1.step(w.b, f, t, lane, has_prev, prev, any, last);
    r2.step(w.c, f, t, lane, has_prev, prev, any, last);
    r3.step(w.d, f, t, lane, has_prev, prev, any, last);
  }
  const BootPartial p0 = r0.close(), p1 = r1.close(), p2 = r2.close(), p3 = r3.close();
  if (lane == 0) {
    BootPartial* dst = part + ((int64_t)s * Q + q) * 4;
    dst[0] = p0;
    dst[1] = p1;
    dst[2] = p2;
    dst[3] = p3;
  }
}

__global__ void __launch_bounds__(256) boot_close_kernel(const BootPartial* __restrict__ part, int S, int Q, int R,
                                                         unsigned long long* __restrict__ u2,
                                                         unsigned long long* __restrict__ pos_w,
                                                         unsigned long long* __restrict__ neg_w,
                                                         double* __restrict__ sum_loss) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  unsigned long long u = 0, pw = 0, nw = 0;
  double l = 0.0;
  for (int s = 0; s < S; ++s) {
    const BootPartial p = part[(int64_t)s * Q * 4 + r];
    u += p.a + 2ull * p.pos * nw;
    pw += p.pos;
    nw += p.neg;
    l += p.loss;
  }
  u2[r] = u;
  pos_w[r] = pw;
  neg_w[r] = nw;
  sum_loss[r] = l;
}

static size_t boot_align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct BootLayout {
  size_t keys_in, keys_out, rows_in, rows_out, unit, term, flag, starts, part, temp, temp_bytes, total;
  int S, Q;
  int64_t L;
};

static BootLayout boot_layout(int64_t n, int R) {
  BootLayout B{};
  (void)rocprim::radix_sort_pairs(nullptr, B.temp_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, kBootProbBits,
                                  hipStream_t(0));
  B.L = boot_segment_rows(n);
  B.S = boot_segments(n);
  B.Q = (R + 3) / 4;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += boot_align256(bytes); return o; };
  B.keys_in = take((size_t)n * 4);
  B.keys_out = take((size_t)n * 4);
  B.rows_in = take((size_t)n * 4);
  B.rows_out = take((size_t)n * 4);
  B.unit = take((size_t)n * 8);
  B.term = take((size_t)n * 8);
  B.flag = take((size_t)n);
  B.starts = take((size_t)(B.S + 1) * 8);
  B.part = take((size_t)B.S * B.Q * 4 * sizeof(BootPartial));
  B.temp = take(B.temp_bytes);
  B.total = off;
  return B;
}

static bool boot_sizes_ok(int64_t n, int R) {
  return n >= 1 && n <= kBootMaxRows && R >= 1 && R <= kBootMaxReplicates;
}

}  // namespace mapx

extern "C" size_t mapx_bootstrap_workspace_bytes(int64_t n, int replicates) {
  return mapx::boot_sizes_ok(n, replicates) ? mapx::boot_layout(n, replicates).total : 256;
}

extern "C" int mapx_bootstrap_metrics(const float* logits, const float* labels, const int64_t* units, int64_t n,
                                      int replicates, uint64_t seed, uint64_t* u2, uint64_t* pos_w, uint64_t* neg_w,
                                      double* sum_loss, void* ws, size_t ws_bytes, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 1 && n <= kBootMaxRows, "bootstrap_metrics: 1 to 2^28 rows (n = %lld)", (long long)n);
  MAPX_REQUIRE(replicates >= 1 && replicates <= kBootMaxReplicates, "bootstrap_metrics: 1 to 65536 replicates (R = %d)",
               replicates);
  MAPX_REQUIRE(logits && labels && u2 && pos_w && neg_w && sum_loss && ws, "bootstrap_metrics: null pointer");
  const BootLayout B = boot_layout(n, replicates);
  if (ws_bytes < B.total) {
    set_error("bootstrap_metrics: workspace %zu B < %zu B", ws_bytes, B.total);
    return MAPX_EWORKSPACE;
  }
  char* base = static_cast<char*>(ws);
  uint32_t* keys_in = reinterpret_cast<uint32_t*>(base + B.keys_in);
  uint32_t* keys = reinterpret_cast<uint32_t*>(base + B.keys_out);
  uint32_t* rows_in = reinterpret_cast<uint32_t*>(base + B.rows_in);
  uint32_t* rows = reinterpret_cast<uint32_t*>(base + B.rows_out);
  uint64_t* unit = reinterpret_cast<uint64_t*>(base + B.unit);
  double* term = reinterpret_cast<double*>(base + B.term);
  uint8_t* flag = reinterpret_cast<uint8_t*>(base + B.flag);
  int64_t* starts = reinterpret_cast<int64_t*>(base + B.starts);
  BootPartial* part = reinterpret_cast<BootPartial*>(base + B.part);
  hipLaunchKernelGGL(boot_prepare_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, logits, n, keys_in, rows_in);
  size_t tb = B.temp_bytes;
  MAPX_HIP(rocprim::radix_sort_pairs(base + B.temp, tb, keys_in, keys, rows_in, rows, (size_t)n, 0u, kBootProbBits,
                                     stream));
  hipLaunchKernelGGL(boot_rows_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, keys, rows, labels, units, n,
                     unit, flag, term);
  hipLaunchKernelGGL(boot_borders_kernel, dim3(B.S + 1), dim3(kWave), 0, stream, flag, n, B.L, B.S, starts);
  hipLaunchKernelGGL(boot_replicate_kernel, dim3((B.Q + 3) / 4, B.S), dim3(256), 0, stream, unit, flag, term, starts,
                     B.Q, seed, part);
  hipLaunchKernelGGL(boot_close_kernel, dim3((replicates + 255) / 256), dim3(256), 0, stream, part, B.S, B.Q,
                     replicates, reinterpret_cast<unsigned long long*>(u2),
                     reinterpret_cast<unsigned long long*>(pos_w), reinterpret_cast<unsigned long long*>(neg_w),
                     sum_loss);
  return check_launch("bootstrap_metrics");
}

extern "C" int mapx_bootstrap_weights(const int64_t* units, int64_t n, int replicates, uint64_t seed, uint8_t* w,
                                      hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 1 && n <= kBootMaxRows, "bootstrap_weights: 1 to 2^28 rows (n = %lld)", (long long)n);
  MAPX_REQUIRE(replicates >= 1 && replicates <= kBootMaxReplicates, "bootstrap_weights: 1 to 65536 replicates (R = %d)",
               replicates);
  MAPX_REQUIRE(w, "bootstrap_weights: null pointer");
  hipLaunchKernelGGL(boot_weights_kernel, dim3(grid_for(n, 256), (replicates + 3) / 4), dim3(256), 0, stream, units, n,
                     replicates, seed, w);
  return check_launch("bootstrap_weights");
}
