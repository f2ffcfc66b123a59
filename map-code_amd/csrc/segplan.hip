// Segment plan: sort n int32 keys (table row ids) and describe the runs of equal keys.
// Built once per step per table from the ids alone, BEFORE the forward pass, so the same
// plan serves the lazy-optimizer catch-up of the touched rows (optim.hip) and the
// deterministic gradient reduce-by-key after the backward pass (segreduce.h).
//
// The sort is the hand-written LSD radix sort of radixsort.h (8-bit digits: two launches per pass, two more for the
// runs; 9- and 12-bit digits and a scan launch per pass were measured and lost).  Its kernels take a list of
// problems; the three plan entries below fill that list (add_prob) and share one launch routine: mapx_seg_plan is
// the one-problem case of mapx_seg_plan_multi, mapx_seg_plan_merge a ranking launch in place of the sort passes.
#include <cstdlib>
#include <cstring>

#include "../../include/mapx_hip.h"
#include "common.h"
#include "radixsort.h"
#include "segreduce.h"

namespace mapx {

static inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

static int key_bits_for(int64_t V) {
  int b = 1;
  while (((int64_t)1 << b) < V && b < 31) ++b;
  return b;
}

// Carve-up of the caller's workspace for one problem, from byte `at` on: two ping-pong arrays, the
// histogram matrix of the running pass, the tile counts of the run kernels.
struct ProbWs {
  size_t tk, tv, bh, cnt, end;
};
static ProbWs prob_ws(int64_t n, size_t at) {
  ProbWs w;
  size_t o = at;
  auto take = [&](size_t bytes) { size_t a = o; o = align_up(o + bytes); return a; };
  const size_t hist = (size_t)(1 << kSortBits) * radix_ld(radix_blocks(n));
  w.tk = take((size_t)n * 4);
  w.tv = take((size_t)n * 4);
  w.bh = take(hist * 4);
  w.cnt = take((size_t)radix_blocks(n) * 4);
  w.end = o;
  return w;
}
static size_t plan_ws_bytes(int count, const int64_t* n) {
  size_t at = 0;
  for (int q = 0; q < count; ++q)
    if (n[q] > 0) at = prob_ws(n[q], at).end;
  return at + 256;
}

struct PlanOut {   // the arrays of one plan (include/mapx_hip.h)
  int32_t *sorted_keys, *perm, *rank, *uniq, *seg_start, *n_uniq;
};

// Appends the problem {keys[n] of `bits` bits -> o} to ps, its scratch carved from the workspace at byte
// `at`.  An empty list gets its plan, {0 runs}, here and takes no part in the launches.  `what` names the
// entry in the error messages.
static int add_prob(SortProbs& ps, size_t& at, const char* what, const int32_t* keys, int64_t n, int bits,
                    void* ws, size_t ws_bytes, const PlanOut& o, hipStream_t stream) {
  MAPX_REQUIRE(o.n_uniq && o.seg_start, "%s: null output", what);
  if (n == 0) {
    MAPX_HIP(hipMemsetAsync(o.n_uniq, 0, 2 * sizeof(int32_t), stream));
    MAPX_HIP(hipMemsetAsync(o.seg_start, 0, sizeof(int32_t), stream));
    return MAPX_OK;
  }
  MAPX_REQUIRE(keys && o.sorted_keys && o.perm && o.rank && o.uniq && ws, "%s: null pointer", what);
  MAPX_REQUIRE((uintptr_t)ws % 256 == 0, "%s: workspace must be 256-byte aligned", what);
  SortProb& pr = ps.p[ps.count];
  pr.keys = keys; pr.n = n;
  pr.nblocks = radix_blocks(n);
  pr.block0 = ps.count ? ps.p[ps.count - 1].block0 + ps.p[ps.count - 1].nblocks : 0;
  pr.bits = bits; pr.passes = radix_passes(bits);
  MAPX_REQUIRE(pr.passes <= kMaxPasses, "%s: keys wider than %d bits", what, kMaxPasses * kSortBits);
  const ProbWs w = prob_ws(n, at);
  if (ws_bytes < w.end) {
    set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w.end);
    return MAPX_EWORKSPACE;
  }
  at = w.end;
  char* base = static_cast<char*>(ws);
  pr.tk = reinterpret_cast<int32_t*>(base + w.tk);
  pr.tv = reinterpret_cast<int32_t*>(base + w.tv);
  pr.bh = reinterpret_cast<int32_t*>(base + w.bh);
  pr.cnt = reinterpret_cast<int32_t*>(base + w.cnt);
  pr.sorted_keys = o.sorted_keys; pr.perm = o.perm; pr.rank = o.rank; pr.uniq = o.uniq;
  pr.seg_start = o.seg_start; pr.n_uniq = o.n_uniq;
  ++ps.count;
  return MAPX_OK;
}

static int sort_blocks(const SortProbs& ps) { return ps.p[ps.count - 1].block0 + ps.p[ps.count - 1].nblocks; }

// The runs of equal keys in every problem's sorted_keys: rank, uniq, seg_start, n_uniq.
static int launch_runs(const SortProbs& ps, hipStream_t stream, const char* what) {
  if (ps.count == 0) return MAPX_OK;
  const int blocks = sort_blocks(ps);
  const RunProbs rp = run_probs_of(ps);
  hipLaunchKernelGGL(seg_count_mp_kernel, dim3(blocks), dim3(256), 0, stream, rp);
  hipLaunchKernelGGL(seg_mark_mp_kernel, dim3(blocks), dim3(256), 0, stream, rp);
  return check_launch(what);
}

// The whole plan of every problem: the sort passes of the widest keys (a problem with narrower keys sits
// out the passes it does not need), then the runs.
static int launch_sort_and_runs(const SortProbs& ps, hipStream_t stream, const char* what) {
  if (ps.count == 0) return MAPX_OK;
  const int blocks = sort_blocks(ps);
  int max_passes = 0;
  for (int q = 0; q < ps.count; ++q)
    if (ps.p[q].passes > max_passes) max_passes = ps.p[q].passes;
  for (int p = 0; p < max_passes; ++p) {
    hipLaunchKernelGGL(radix_hist_mp_kernel, dim3(blocks), dim3(256), 0, stream, ps, p);
    if (p == 0) hipLaunchKernelGGL(radix_scatter_mp_kernel<true>, dim3(blocks), dim3(256), 0, stream, ps, p);
    else hipLaunchKernelGGL(radix_scatter_mp_kernel<false>, dim3(blocks), dim3(256), 0, stream, ps, p);
  }
  return launch_runs(ps, stream, what);
}
}  // namespace mapx

// V does not enter the layout (the merge form passes 0).
extern "C" size_t mapx_seg_plan_workspace_bytes(int64_t n, int64_t V) {
  (void)V;
  return mapx::plan_ws_bytes(1, &n);
}

extern "C" size_t mapx_seg_plan_multi_workspace_bytes(int count, const int64_t* n, const int64_t* V) {
  (void)V;
  return mapx::plan_ws_bytes(count, n);
}

// The plans of up to kMaxSortProbs key lists (the step's tables) from ONE chain of launches.
extern "C" int mapx_seg_plan_multi(int count, const int32_t* const* keys, const int64_t* n, const int64_t* V,
                                   void* ws, size_t ws_bytes, int32_t* const* sorted_keys, int32_t* const* perm,
                                   int32_t* const* rank, int32_t* const* uniq, int32_t* const* seg_start,
                                   int32_t* const* n_uniq, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(count >= 1 && count <= kMaxSortProbs, "seg_plan_multi: 1..%d key lists per call", kMaxSortProbs);
  MAPX_REQUIRE(keys && n && V && sorted_keys && perm && rank && uniq && seg_start && n_uniq, "seg_plan_multi: null array");
  SortProbs ps;
  memset(&ps, 0, sizeof(ps));
  size_t at = 0;
  for (int q = 0; q < count; ++q) {
    MAPX_REQUIRE(n[q] >= 0 && n[q] < (1LL << 31) && V[q] > 0 && V[q] < (1LL << 31), "seg_plan_multi: bad sizes");
    const PlanOut o{sorted_keys[q], perm[q], rank[q], uniq[q], seg_start[q], n_uniq[q]};
    const int rc = add_prob(ps, at, "seg_plan_multi", keys[q], n[q], key_bits_for(V[q]), ws, ws_bytes, o, stream);
    if (rc != MAPX_OK) return rc;
  }
  return launch_sort_and_runs(ps, stream, "seg_plan_multi");
}

// One key list: the one-problem case of the above.
extern "C" int mapx_seg_plan(const int32_t* keys, int64_t n, int64_t V, void* ws, size_t ws_bytes,
                             int32_t* sorted_keys, int32_t* perm, int32_t* rank, int32_t* uniq,
                             int32_t* seg_start, int32_t* n_uniq, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 0 && n < (1LL << 31) && V > 0 && V < (1LL << 31), "seg_plan: bad sizes");
  SortProbs ps;
  memset(&ps, 0, sizeof(ps));
  size_t at = 0;
  const PlanOut o{sorted_keys, perm, rank, uniq, seg_start, n_uniq};
  const int rc = add_prob(ps, at, "seg_plan", keys, n, key_bits_for(V), ws, ws_bytes, o, stream);
  if (rc != MAPX_OK) return rc;
  return launch_sort_and_runs(ps, stream, "seg_plan");
}

namespace mapx {
// rank of every key of `lists` sorted lists in their stable merge
__global__ void __launch_bounds__(256) merge_rank_kernel(const int32_t* __restrict__ keys, int lists,
                                                         int64_t len, int32_t* __restrict__ sorted_keys,
                                                         int32_t* __restrict__ perm) {
  const int64_t n = (int64_t)lists * len;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / len);
    const uint32_t k = (uint32_t)keys[e];
    int64_t pos = e - (int64_t)r * len;
    for (int q = 0; q < lists; ++q) {
      if (q == r) continue;
      const int32_t* __restrict__ L = keys + (int64_t)q * len;
      int64_t lo = 0, hi = len;            // q < r: #{L <= k};  q > r: #{L < k}
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const uint32_t v = (uint32_t)L[mid];
        const bool left = q < r ? v <= k : v < k;
        lo = left ? mid + 1 : lo;
        hi = left ? hi : mid;
      }
      pos += lo;
    }
    sorted_keys[pos] = (int32_t)k;
    perm[pos] = (int32_t)e;
  }
}
}  // namespace mapx

// The order comes from one ranking launch; the runs from the run kernels on a one-problem list.
extern "C" int mapx_seg_plan_merge(const int32_t* keys, int lists, int64_t len, void* ws, size_t ws_bytes,
                                   int32_t* sorted_keys, int32_t* perm, int32_t* rank, int32_t* uniq,
                                   int32_t* seg_start, int32_t* n_uniq, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(lists >= 1 && len >= 0 && (int64_t)lists * len < (1LL << 31), "seg_plan_merge: bad sizes");
  const int64_t n = (int64_t)lists * len;
  SortProbs ps;
  memset(&ps, 0, sizeof(ps));
  size_t at = 0;
  const PlanOut o{sorted_keys, perm, rank, uniq, seg_start, n_uniq};
  const int rc = add_prob(ps, at, "seg_plan_merge", keys, n, /*bits=*/0, ws, ws_bytes, o, stream);   // no sort pass
  if (rc != MAPX_OK || ps.count == 0) return rc;
  hipLaunchKernelGGL(merge_rank_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, keys, lists, len,
                     sorted_keys, perm);
  return launch_runs(ps, stream, "seg_plan_merge");
}

// Generic reduce-by-key of dense rows: out[u, :] = sum over the positions of key uniq[u] of
// src[position, :], in sorted-position order.  Embedding-table gradient: src = dL/dX0
// viewed as [B*F, E], keys = input_ids.flatten() (reference: aten::embedding_dense_backward).
extern "C" size_t mapx_seg_reduce_workspace_bytes(int64_t n, int W) {
  return mapx::seg_reduce_partial_bytes(n, W, true) + 256;
}

namespace mapx {
// The entries below for T = float (rows read with 16-byte loads) and T = __bf16 (8-byte loads).
template <class T>
constexpr unsigned kRowAlign = sizeof(T) * 4;
template <class T>
constexpr const char* kRowAlignMsg =
    sizeof(T) == 4 ? "%s: pointers must be 16-byte aligned" : "%s: pointers must be 8 / 16-byte aligned";

template <class T>
static int reduce_rows(const char* what, int64_t n, const int32_t* perm, const int32_t* rank,
                       const int32_t* seg_start, const T* src, const T* src2_opt, int W, float* out, void* ws,
                       size_t ws_bytes, int32_t* zeroed_counter_opt, hipStream_t stream) {
  MAPX_REQUIRE(n >= 0, "%s: n < 0", what);
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(perm && rank && seg_start && src && out, "%s: null pointer", what);
  MAPX_REQUIRE((uintptr_t)src % kRowAlign<T> == 0 && (uintptr_t)src2_opt % kRowAlign<T> == 0 &&
                   (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0,
               kRowAlignMsg<T>, what);
  SegPlanView pl{n, perm, rank, seg_start};
  if (src2_opt) {
    RowsContrib<T, true> c2{{src, src2_opt}, W};
    return seg_reduce_launch<false>(pl, c2, W, out, nullptr, ws, ws_bytes, zeroed_counter_opt, stream, what);
  }
  RowsContrib<T, false> c{{src}, W};
  return seg_reduce_launch<false>(pl, c, W, out, nullptr, ws, ws_bytes, zeroed_counter_opt, stream, what);
}

template <class T>
static int reduce_rows_extra(const char* what, int64_t n, const int32_t* perm, const int32_t* rank,
                             const int32_t* seg_start, const T* src, int W, int64_t ld_src, const float* extra,
                             int group, int64_t extra_stride, float* out, float* out_extra, void* ws,
                             size_t ws_bytes, int32_t* zeroed_counter_opt, hipStream_t stream) {
  MAPX_REQUIRE(n >= 0 && group >= 1 && ld_src >= W && ld_src % 4 == 0 && extra_stride >= 1, "%s: bad sizes", what);
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(perm && rank && seg_start && src && extra && out && out_extra, "%s: null pointer", what);
  MAPX_REQUIRE((uintptr_t)src % kRowAlign<T> == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0,
               kRowAlignMsg<T>, what);
  SegPlanView pl{n, perm, rank, seg_start};
  RowsExtraContrib<T> c{src, W, ld_src, extra, group, extra_stride};
  return seg_reduce_launch<true>(pl, c, W, out, out_extra, ws, ws_bytes, zeroed_counter_opt, stream, what);
}
}  // namespace mapx

extern "C" int mapx_seg_reduce_rows(int64_t n, const int32_t* perm, const int32_t* rank,
                                    const int32_t* seg_start, const float* src, const float* src2_opt, int W,
                                    float* out, void* ws, size_t ws_bytes, int32_t* zeroed_counter_opt,
                                    hipStream_t stream) {
  return mapx::reduce_rows("seg_reduce_rows", n, perm, rank, seg_start, src, src2_opt, W, out, ws, ws_bytes,
                           zeroed_counter_opt, stream);
}

// mapx_seg_reduce_rows over bf16 gradient rows: fp32 sums and output.
extern "C" int mapx_seg_reduce_rows_bf16(int64_t n, const int32_t* perm, const int32_t* rank,
                                         const int32_t* seg_start, const mapx_bf16* src, const mapx_bf16* src2_opt,
                                         int W, float* out, void* ws, size_t ws_bytes,
                                         int32_t* zeroed_counter_opt, hipStream_t stream) {
  return mapx::reduce_rows("seg_reduce_rows_bf16", n, perm, rank, seg_start, reinterpret_cast<const __bf16*>(src),
                           reinterpret_cast<const __bf16*>(src2_opt), W, out, ws, ws_bytes, zeroed_counter_opt,
                           stream);
}

// Same reduction with an extra scalar per run: out_extra[u] = sum over the run of
// extra[position / group] (DeepFM: the LR weight shares the embedding's ids, its gradient
// dL/dlr[b] is common to the F positions of batch row b).
extern "C" int mapx_seg_reduce_rows_extra(int64_t n, const int32_t* perm, const int32_t* rank,
                                          const int32_t* seg_start, const float* src, int W, int64_t ld_src,
                                          const float* extra, int group, int64_t extra_stride, float* out,
                                          float* out_extra,
                                          void* ws, size_t ws_bytes, int32_t* zeroed_counter_opt,
                                          hipStream_t stream) {
  return mapx::reduce_rows_extra("seg_reduce_rows_extra", n, perm, rank, seg_start, src, W, ld_src, extra, group,
                                 extra_stride, out, out_extra, ws, ws_bytes, zeroed_counter_opt, stream);
}

// mapx_seg_reduce_rows_extra over bf16 rows: the same plan order, fp32 sums and outputs, the scalar fp32.
extern "C" int mapx_seg_reduce_rows_extra_bf16(int64_t n, const int32_t* perm, const int32_t* rank,
                                               const int32_t* seg_start, const mapx_bf16* src, int W, int64_t ld_src,
                                               const float* extra, int group, int64_t extra_stride, float* out,
                                               float* out_extra, void* ws, size_t ws_bytes,
                                               int32_t* zeroed_counter_opt, hipStream_t stream) {
  return mapx::reduce_rows_extra("seg_reduce_rows_extra_bf16", n, perm, rank, seg_start,
                                 reinterpret_cast<const __bf16*>(src), W, ld_src, extra, group, extra_stride, out,
                                 out_extra, ws, ws_bytes, zeroed_counter_opt, stream);
}

// Data-parallel exchange (mapx/parallel.py): the first n_uniq (id, gradient row) pairs of a rank's
// sparse gradient as a fixed-size message of `maxc` entries: keys_out[i] = uniq[i], rows_out[i] =
// {rows0[i, :] * scale, rows1[i] * scale, 0, 0, 0} (rows1 optional: then W0 columns only); entries
// at and beyond *n_uniq are id `pad_id` with a zero row.  One launch instead of a dozen tensor ops.
namespace mapx {
__global__ void __launch_bounds__(256) pack_sparse_kernel(const int32_t* __restrict__ uniq,
                                                          const float* __restrict__ rows0, int W0,
                                                          const float* __restrict__ rows1,
                                                          const int32_t* __restrict__ n_uniq, int64_t cap,
                                                          int64_t maxc, float scale, int32_t pad_id,
                                                          int32_t* __restrict__ keys_out,
                                                          float* __restrict__ rows_out) {
  const int Wp = rows1 ? W0 + 4 : W0;
  const int per = Wp / 4;
  int64_t n = *n_uniq;
  if (n > cap) n = cap;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < maxc * per;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / per;
    const int c = (int)(t - i * per) * 4;
    const bool live = i < n;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      if (c < W0) {
        v = *reinterpret_cast<const float4*>(rows0 + i * W0 + c);
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
      } else {
        v.x = rows1[i] * scale;
      }
    }
    *reinterpret_cast<float4*>(rows_out + i * Wp + c) = v;
    if (c == 0) keys_out[i] = live ? uniq[i] : pad_id;
  }
}
__global__ void __launch_bounds__(64) publish_i32_kernel(const int32_t* __restrict__ src, int n,
                                                         int32_t* __restrict__ stamp,
                                                         volatile int32_t* __restrict__ host_out) {
  const int lane = threadIdx.x;
  int v = lane < n ? src[lane] : 0;
  if (lane < n) host_out[lane] = v;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  __threadfence_system();
  if (lane == 0) {
    const int s = *stamp + 1;
    *stamp = s;
    __hip_atomic_store((int32_t*)host_out + n + 1, v + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store((int32_t*)host_out + n, s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace mapx

extern "C" int mapx_pack_sparse(const int32_t* uniq, const float* rows0, int W0, const float* rows1_opt,
                                const int32_t* n_uniq, int64_t cap, int64_t maxc, float scale,
                                int32_t pad_id, int32_t* keys_out, float* rows_out, hipStream_t stream) {
  MAPX_REQUIRE(W0 > 0 && W0 % 4 == 0 && cap >= 0 && maxc >= 0, "pack_sparse: bad sizes");
  if (maxc == 0) return MAPX_OK;          // an empty message: its outputs have no storage to point at
  MAPX_REQUIRE(uniq && rows0 && n_uniq && keys_out && rows_out, "pack_sparse: null pointer");
  const int Wp = rows1_opt ? W0 + 4 : W0;
  hipLaunchKernelGGL(mapx::pack_sparse_kernel, dim3(mapx::grid_for(maxc * (Wp / 4), 256)), dim3(256), 0, stream,
                     uniq, rows0, W0, rows1_opt, n_uniq, cap, maxc, scale, pad_id, keys_out, rows_out);
  return mapx::check_launch("pack_sparse");
}

extern "C" int mapx_publish_i32(const int32_t* src, int n, int32_t* stamp_dev, int32_t* host_out,
                                hipStream_t stream) {
  MAPX_REQUIRE(src && stamp_dev && host_out, "publish_i32: null pointer");
  MAPX_REQUIRE(n >= 0 && n <= 64, "publish_i32: n must be in [0, 64]");
  hipLaunchKernelGGL(mapx::publish_i32_kernel, dim3(1), dim3(64), 0, stream, src, n, stamp_dev, host_out);
  return mapx::check_launch("publish_i32");
}
