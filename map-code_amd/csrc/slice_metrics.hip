// Sliced evaluation on the device: per group g of a column of group ids, the counts and sums from which the host
// forms AUC, GAUC, log-loss and calibration per slice (mapx/score.py: slice_report).
//
//   rows[g], positives[g]   exact counts
//   u2[g]                   twice the U statistic of metrics.hip's header, taken inside the group: a positive ranked
//                           above a negative of the same group counts 2, a tie of their fp32 probabilities counts 1
//   sum_prob[g]             sum of (double)sigmoid_f32(logit)
//   sum_loss[g]             sum of eval_prepare_kernel's row terms, the same clip eps = 2^-52
//
// One 64-bit key per row,  group << 31 | bits(p32) << 1 | positive,  is ALL the later launches read: p32 and the
// label come back out of the sorted key, so the sorted sequence is a function of the multiset of rows, not of their
// input order, and so is everything below.  Launches:
//   1. slice_prepare_kernel   keys; a group id outside [0, G) is counted (a compare, never an access) and its row
//                             filed under group 0
//   2. rocprim::radix_sort_keys over the low 31 + bit_length(G - 1) bits
//   3. rocprim::inclusive_scan of {negatives so far, tie-run start, group start} (two max-fields)
//   4. slice_chunk_kernel     chunks of 256 sorted rows: rows / positives at each group's last row from the scan state
//                             alone; one term per tie run; a group wholly inside a chunk is summed there in row order;
//                             the pieces of a group that leaves the chunk go to head[chunk] / tail[chunk]
//   5. slice_close_kernel     one wave per chunk closes the groups that START in it and span chunks: lane l adds
//                             head[first + l], head[first + l + 64], ... in order, a fixed shuffle tree adds the
//                             lanes, the first chunk's tail is added in front
// No floating-point atomics and no look-back: every fp64 addition's place is fixed by the sorted sequence.  The only
// atomics are the two integer ones of the refusal path in launch 1.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

constexpr int kSliceChunk = 256;
constexpr unsigned kSliceProbBits = 30;                       // fp32 values in [0, 1] have bit patterns < 2^30
constexpr unsigned kSliceGroupShift = kSliceProbBits + 1;     // bit 0 is the label
constexpr uint32_t kSliceOneBits = 0x3F800000u;

struct SliceState {
  int32_t neg;   // negatives among the sorted rows [0, i]
  int32_t run;   // index where the tie run containing i starts
  int32_t grp;   // index where the group containing i starts
};
struct SliceCombine {
  __host__ __device__ SliceState operator()(const SliceState& a, const SliceState& b) const {
    return SliceState{a.neg + b.neg, a.run > b.run ? a.run : b.run, a.grp > b.grp ? a.grp : b.grp};
  }
};
struct SliceInput {
  const uint64_t* keys;
  __host__ __device__ SliceState operator()(int32_t i) const {
    const uint64_t k = keys[i], prev = i > 0 ? keys[i - 1] : 0;
    const bool run_head = (i == 0) || ((k >> 1) != (prev >> 1));
    const bool grp_head = (i == 0) || ((k >> kSliceGroupShift) != (prev >> kSliceGroupShift));
    return SliceState{(int32_t)(~k & 1), run_head ? i : 0, grp_head ? i : 0};
  }
};

struct SlicePartial {
  unsigned long long u2;
  double prob, loss;
};

// status[0] = rows whose group id lies outside [0, G), status[1] = the first such row (all ones when there is none).
__global__ void __launch_bounds__(256) slice_prepare_kernel(const float* __restrict__ logits,
                                                            const float* __restrict__ labels,
                                                            const int32_t* __restrict__ groups, int64_t n, int64_t G,
                                                            uint64_t* __restrict__ keys,
                                                            unsigned long long* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int32_t g = groups[i];
    if (g < 0 || (int64_t)g >= G) {
      atomicAdd(&status[0], 1ull);
      atomicMin(&status[1], (unsigned long long)i);
      g = 0;
    }
    uint32_t bits = __float_as_uint(sigmoid_f32(logits[i]));
    bits = bits > kSliceOneBits ? kSliceOneBits : bits;   // (a NaN logit must not reach the group bits: it ranks as 1)
    keys[i] = ((uint64_t)(uint32_t)g << kSliceGroupShift) | ((uint64_t)bits << 1) | (labels[i] > 0.5f ? 1u : 0u);
  }
}

// One block per chunk of 256 sorted rows, one row per thread.
__global__ void __launch_bounds__(kSliceChunk) slice_chunk_kernel(
    const uint64_t* __restrict__ keys, const SliceState* __restrict__ st, int64_t n, int64_t* __restrict__ rows,
    int64_t* __restrict__ positives, unsigned long long* __restrict__ u2, double* __restrict__ sum_prob,
    double* __restrict__ sum_loss, SlicePartial* __restrict__ head, SlicePartial* __restrict__ tail) {
  __shared__ unsigned long long s_u[kSliceChunk];
  __shared__ double s_p[kSliceChunk], s_l[kSliceChunk];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kSliceChunk, i = base + t;
  const bool live = i < n;
  SliceState e{0, 0, 0};
  int64_t g = 0;
  bool grp_last = false;
  if (live) {
    const uint64_t k = keys[i], next = i + 1 < n ? keys[i + 1] : 0;
    const bool run_last = (i == n - 1) || ((next >> 1) != (k >> 1));
    g = (int64_t)(k >> kSliceGroupShift);
    grp_last = (i == n - 1) || ((int64_t)(next >> kSliceGroupShift) != g);
    e = st[i];
    const bool y = (k & 1) != 0;
    const double p = (double)__uint_as_float((uint32_t)(k >> 1) & ((1u << kSliceProbBits) - 1u));
    const double eps = 2.220446049250313e-16;
    double q = y ? p : 1.0 - p;
    q = q < eps ? eps : (q > 1.0 - eps ? 1.0 - eps : q);
    unsigned long long term = 0;
    if (run_last) {   // (a group's last row ends a tie run too)
      const int64_t neg_grp = e.grp > 0 ? st[e.grp - 1].neg : 0;
      const int64_t neg_before = (e.run > 0 ? st[e.run - 1].neg : 0) - neg_grp;
      const int64_t neg_through = e.neg - neg_grp;
      const int64_t pos_run = (i - e.run + 1) - (neg_through - neg_before);
      term = (unsigned long long)pos_run * (unsigned long long)(neg_before + neg_through);
      if (grp_last) {
        rows[g] = i - e.grp + 1;
        positives[g] = (i - e.grp + 1) - neg_through;
      }
    }
    s_u[t] = term;
    s_p[t] = p;
    s_l[t] = -log(q);
  }
  __syncthreads();
  const bool chunk_last = (t == kSliceChunk - 1) || (i == n - 1);
  if (!live || !(grp_last || chunk_last)) return;
  // this row ends a group's piece inside the chunk: sum the piece in row order
  const int lo = e.grp > base ? (int)(e.grp - base) : 0;
  unsigned long long u = 0;
  double sp = 0.0, sl = 0.0;
  for (int j = lo; j <= t; ++j) {
    u += s_u[j];
    sp += s_p[j];
    sl += s_l[j];
  }
  if (grp_last && e.grp >= base) {          // the whole group lies in this chunk
    u2[g] = u;
    sum_prob[g] = sp;
    sum_loss[g] = sl;
  } else if (e.grp <= base) {               // the piece holds the chunk's first row
    head[blockIdx.x] = SlicePartial{u, sp, sl};
  } else {                                  // it began inside the chunk and goes on behind it
    tail[blockIdx.x] = SlicePartial{u, sp, sl};
  }
}

// A group of chunks [first, last] (its head pieces) behind an optional tail piece; one wave, lane 0 stores.
__device__ inline void slice_close_group(int lane, int64_t g, const SlicePartial* tail_opt, int64_t first, int64_t last,
                                         const SlicePartial* __restrict__ head, unsigned long long* __restrict__ u2,
                                         double* __restrict__ sum_prob, double* __restrict__ sum_loss) {
  unsigned long long u = 0;
  double sp = 0.0, sl = 0.0;
  for (int64_t c = first + lane; c <= last; c += kWave) {
    const SlicePartial h = head[c];
    u += h.u2;
    sp += h.prob;
    sl += h.loss;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    u += __shfl_down(u, off);
    sp += __shfl_down(sp, off);
    sl += __shfl_down(sl, off);
  }
  if (lane != 0) return;
  if (tail_opt) {
    u = tail_opt->u2 + u;
    sp = tail_opt->prob + sp;
    sl = tail_opt->loss + sl;
  }
  u2[g] = u;
  sum_prob[g] = sp;
  sum_loss[g] = sl;
}

// Wave c closes the (at most two) groups that start in chunk c and do not end in it: the one that starts at the
// chunk's first row, and the one that holds its last row.  Every branch is uniform over the wave.
__global__ void __launch_bounds__(kWave) slice_close_kernel(
    const uint64_t* __restrict__ keys, const SliceState* __restrict__ st, int64_t n, const int64_t* __restrict__ rows,
    const SlicePartial* __restrict__ head, const SlicePartial* __restrict__ tail, unsigned long long* __restrict__ u2,
    double* __restrict__ sum_prob, double* __restrict__ sum_loss) {
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x, i0 = c * kSliceChunk;
  const int64_t r = i0 + kSliceChunk - 1 < n - 1 ? i0 + kSliceChunk - 1 : n - 1;
  if (st[i0].grp == i0) {
    const int64_t g = (int64_t)(keys[i0] >> kSliceGroupShift);
    const int64_t end = i0 + rows[g];
    if (end > i0 + kSliceChunk)
      slice_close_group(lane, g, nullptr, c, (end - 1) / kSliceChunk, head, u2, sum_prob, sum_loss);
  }
  const int64_t s = st[r].grp;
  if (s > i0 && r < n - 1) {
    const int64_t g = (int64_t)(keys[r] >> kSliceGroupShift);
    if ((int64_t)(keys[r + 1] >> kSliceGroupShift) == g)
      slice_close_group(lane, g, &tail[c], c + 1, (s + rows[g] - 1) / kSliceChunk, head, u2, sum_prob, sum_loss);
  }
}

static size_t slice_align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct SliceLayout {
  size_t keys_in, keys_out, st, head, tail, temp, temp_bytes, total;
  int64_t chunks;
};

static SliceLayout slice_layout(int64_t n) {
  SliceLayout L{};
  size_t sort_bytes = 0, scan_bytes = 0;
  (void)rocprim::radix_sort_keys(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0u,
                                 64u, hipStream_t(0));
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int32_t>(0), SliceInput{nullptr});
  (void)rocprim::inclusive_scan(nullptr, scan_bytes, in, (SliceState*)nullptr, (size_t)n, SliceCombine(),
                                hipStream_t(0));
  L.chunks = ceil_div(n, kSliceChunk);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += slice_align256(bytes); return o; };
  L.keys_in = take((size_t)n * 8);
  L.keys_out = take((size_t)n * 8);
  L.st = take((size_t)n * sizeof(SliceState));
  L.head = take((size_t)L.chunks * sizeof(SlicePartial));
  L.tail = take((size_t)L.chunks * sizeof(SlicePartial));
  L.temp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
  L.temp = take(L.temp_bytes);
  L.total = off;
  return L;
}

static bool slice_sizes_ok(int64_t n, int64_t n_groups) {
  return n >= 1 && n < ((int64_t)1 << 31) && n_groups >= 1 && n_groups < ((int64_t)1 << 31);
}

}  // namespace mapx

extern "C" size_t mapx_slice_metrics_workspace_bytes(int64_t n, int64_t n_groups) {
  return mapx::slice_sizes_ok(n, n_groups) ? mapx::slice_layout(n).total : 256;
}

extern "C" int mapx_slice_metrics(const float* logits, const float* labels, const int32_t* groups, int64_t n,
                                  int64_t n_groups, int64_t* rows, int64_t* positives, uint64_t* u2, double* sum_prob,
                                  double* sum_loss, int64_t* status2, void* ws, size_t ws_bytes, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "slice_metrics: 1 to 2^31 - 1 rows (n = %lld)", (long long)n);
  MAPX_REQUIRE(n_groups >= 1 && n_groups < ((int64_t)1 << 31), "slice_metrics: 1 to 2^31 - 1 groups (G = %lld)",
               (long long)n_groups);
  MAPX_REQUIRE(logits && labels && groups && rows && positives && u2 && sum_prob && sum_loss && status2 && ws,
               "slice_metrics: null pointer");
  const SliceLayout L = slice_layout(n);
  if (ws_bytes < L.total) {
    set_error("slice_metrics: workspace %zu B < %zu B", ws_bytes, L.total);
    return MAPX_EWORKSPACE;
  }
  char* base = static_cast<char*>(ws);
  uint64_t* keys_in = reinterpret_cast<uint64_t*>(base + L.keys_in);
  uint64_t* keys = reinterpret_cast<uint64_t*>(base + L.keys_out);
  SliceState* st = reinterpret_cast<SliceState*>(base + L.st);
  SlicePartial* head = reinterpret_cast<SlicePartial*>(base + L.head);
  SlicePartial* tail = reinterpret_cast<SlicePartial*>(base + L.tail);
  unsigned long long* u2o = reinterpret_cast<unsigned long long*>(u2);
  unsigned long long* status = reinterpret_cast<unsigned long long*>(status2);
  const size_t out_bytes = (size_t)n_groups * 8;
  MAPX_HIP(hipMemsetAsync(rows, 0, out_bytes, stream));
  MAPX_HIP(hipMemsetAsync(positives, 0, out_bytes, stream));
  MAPX_HIP(hipMemsetAsync(u2, 0, out_bytes, stream));
  MAPX_HIP(hipMemsetAsync(sum_prob, 0, out_bytes, stream));
  MAPX_HIP(hipMemsetAsync(sum_loss, 0, out_bytes, stream));
  MAPX_HIP(hipMemsetAsync(status, 0, 8, stream));
  MAPX_HIP(hipMemsetAsync(status + 1, 0xFF, 8, stream));
  hipLaunchKernelGGL(slice_prepare_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, logits, labels, groups, n,
                     n_groups, keys_in, status);
  unsigned group_bits = 0;
  while (((int64_t)1 << group_bits) < n_groups) ++group_bits;   // bit_length(G - 1)
  size_t tb = L.temp_bytes;
  MAPX_HIP(rocprim::radix_sort_keys(base + L.temp, tb, keys_in, keys, (size_t)n, 0u, kSliceGroupShift + group_bits,
                                    stream));
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int32_t>(0), SliceInput{keys});
  tb = L.temp_bytes;
  MAPX_HIP(rocprim::inclusive_scan(base + L.temp, tb, in, st, (size_t)n, SliceCombine(), stream));
  hipLaunchKernelGGL(slice_chunk_kernel, dim3((unsigned)L.chunks), dim3(kSliceChunk), 0, stream, keys, st, n, rows,
                     positives, u2o, sum_prob, sum_loss, head, tail);
  hipLaunchKernelGGL(slice_close_kernel, dim3((unsigned)L.chunks), dim3(kWave), 0, stream, keys, st, n, rows, head,
                     tail, u2o, sum_prob, sum_loss);
  return check_launch("slice_metrics");
}
