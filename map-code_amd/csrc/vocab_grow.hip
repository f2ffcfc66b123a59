// A saved vocabulary grown on a later file, and the [V, W] tables of a checkpoint moved to the grown id space.
//
// Growing keeps every old id's meaning: per field the saved keys stay where they are in rank order, the values of
// the new file that the saved keys do NOT hold are ranked among themselves by the fit's own rule (descending count,
// ties by first occurrence: Counter(misses).most_common()), those seen at least n_core times are appended, then <oov>.
//
//  count_missing  the fit's counting pass (vocab.hip: vocab_count_kernel) behind a lookup in the saved field's slice
//                 of the lookup tables (vocab_apply.hip): a lane takes a row and probes the slice with plain loads
//                 (the table is constant); only a miss claims a slot of a fresh count table, adds to its count and
//                 lowers its first position.  Integer atomics only: the result does not depend on arrival order.
//                 The missing rows are counted by ballot + popcount per wave, one atomic per workgroup.  The count
//                 table then goes through mapx_vocab_compact / rank_keys / assign unchanged.
//  table_migrate  dst [V_new, W] from src [V_old, W]: a row gather whose source row is COMPUTED from the growth plan
//                 (per field n_old, added, base_old, base_new: F <= 64 entries staged in LDS) instead of read from an
//                 index array: reserved rows copy themselves, rank < n_old reads base_old + rank, added rows and the
//                 new <oov> row read the old <oov> row (or, with `fresh`, the j-th added row overall reads fresh[j]).
//                 The field of a row is found by binary search over base_new.  A group of L lanes (a power of two)
//                 takes a row: 16-byte chunks when W % 4 == 0 and every base and pitch is 16-byte aligned, single
//                 elements otherwise (W = 1: a lane a row, contiguous 4-byte runs).  Four rows are in flight per
//                 lane.  No atomics on data, no RNG: bitwise reproducible.  Only [V_new, W] of dst is written.
#include "../../include/mapx_hip.h"
#include "common.h"
#include "vocab_hash.h"

namespace mapx {

constexpr int kGrowThreads = 256;

__global__ void __launch_bounds__(kGrowThreads) vocab_count_missing_kernel(
    const int64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ saved_tkey,
    const int32_t* __restrict__ saved_trank, int64_t slot0, int64_t slots, int64_t n_saved,
    int64_t* __restrict__ tkey, int32_t* __restrict__ tcount, int32_t* __restrict__ tfirst, int64_t cap,
    int* __restrict__ err, unsigned long long* __restrict__ missing_rows) {
  __shared__ unsigned long long s_missing[kGrowThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  unsigned long long wave_missing = 0;                            // lane 0's copy is the wave's
  // every lane of a wave runs the same number of rounds: the ballot sees the whole wave
  for (int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane; i0 < n;
       i0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = i0 + lane;
    bool missing = false;
    if (i < n) {
      const int64_t k = keys[i];
      if (k == kVocabEmpty) {
        atomicOr(err, 1);
      } else {
        missing = n_saved == 0 || vocab_apply_probe(saved_tkey, saved_trank, slot0, slots, n_saved, k) == (int32_t)n_saved;
        if (missing) {
          uint64_t s;
          if (vocab_claim(tkey, cap, k, &s) == kVocabFull) {      // the caller sized the count table too small
            atomicOr(err, 2);
          } else {
            atomicAdd(tcount + s, 1);
            atomicMin(tfirst + s, (int32_t)i);
          }
        }
      }
    }
    const unsigned long long m = __ballot(missing);
    wave_missing += (unsigned long long)__popcll(m);
  }
  if (lane == 0) s_missing[wave] = wave_missing;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int w = 0; w < kGrowThreads / kWave; ++w) total += s_missing[w];
    if (total) atomicAdd(missing_rows, total);
  }
}

// ---------------------------------------------------------------- table migration
struct MigratePlan {                                              // the per-field arrays, in LDS
  int64_t base_new[MAPX_RT_MAX_FIELDS], base_old[MAPX_RT_MAX_FIELDS], n_old[MAPX_RT_MAX_FIELDS],
      added[MAPX_RT_MAX_FIELDS], fresh_off[MAPX_RT_MAX_FIELDS];
};

// Where row `row` of dst comes from: a pointer to the first element of its source row, or nullptr when the plan
// does not place the row inside src / fresh (the caller writes zeros and raises the error word).
__device__ inline const float* migrate_source(const MigratePlan& p, int F, int64_t row, const float* __restrict__ src,
                                              int64_t ld_src, int64_t V_old, const float* __restrict__ fresh,
                                              int64_t ld_fresh, int64_t n_fresh) {
  int64_t srow;
  if (row < p.base_new[0]) {
    srow = row;                                                   // a reserved id
  } else {
    int lo = 0, hi = F;                                           // the field with base_new[f] <= row < base_new[f + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (p.base_new[mid] <= row) lo = mid; else hi = mid;
    }
    const int64_t rank = row - p.base_new[lo], n = p.n_old[lo], a = p.added[lo];
    if (rank < n) {
      srow = p.base_old[lo] + rank;
    } else if (rank < n + a && fresh) {
      const int64_t j = p.fresh_off[lo] + (rank - n);
      return (j >= 0 && j < n_fresh) ? fresh + j * ld_fresh : nullptr;
    } else if (rank <= n + a) {
      srow = p.base_old[lo] + n;                                  // the old <oov> row
    } else {
      return nullptr;
    }
  }
  return (srow >= 0 && srow < V_old) ? src + srow * ld_src : nullptr;
}

template <class T> __device__ inline T migrate_zero();
template <> __device__ inline float migrate_zero<float>() { return 0.0f; }
template <> __device__ inline float4 migrate_zero<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// T = float4 (16-byte chunks) or float (single elements); log2_lanes: lanes that share a row.
template <class T>
__global__ void __launch_bounds__(kGrowThreads) table_migrate_kernel(
    const float* __restrict__ src, int64_t ld_src, int64_t V_old, float* __restrict__ dst, int64_t ld_dst,
    int64_t V_new, int W, int F, const int64_t* __restrict__ n_old, const int64_t* __restrict__ added,
    const int64_t* __restrict__ base_old, const int64_t* __restrict__ base_new, const float* __restrict__ fresh,
    int64_t ld_fresh, int64_t n_fresh, int log2_lanes, int32_t* __restrict__ err) {
  constexpr int kVec = sizeof(T) / sizeof(float), kRows = 4;
  __shared__ MigratePlan p;
  for (int f = threadIdx.x; f < F; f += kGrowThreads) {
    p.base_new[f] = base_new[f];
    p.base_old[f] = base_old[f];
    p.n_old[f] = n_old[f];
    p.added[f] = added[f];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t off = 0;
    for (int f = 0; f < F; ++f) {
      p.fresh_off[f] = off;
      off += p.added[f];
    }
  }
  __syncthreads();
  const int lanes = 1 << log2_lanes, chunks = W / kVec;
  const int64_t tid = (int64_t)blockIdx.x * kGrowThreads + threadIdx.x;
  const int64_t row_step = ((int64_t)gridDim.x * kGrowThreads) >> log2_lanes;
  const int c0 = (int)(tid & (lanes - 1));
  bool bad = false;
  for (int64_t row0 = tid >> log2_lanes; row0 < V_new; row0 += kRows * row_step) {
    const float* from[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int64_t row = row0 + u * row_step;
      from[u] = nullptr;
      if (row < V_new) {
        from[u] = migrate_source(p, F, row, src, ld_src, V_old, fresh, ld_fresh, n_fresh);
        bad |= from[u] == nullptr;
      }
    }
    for (int c = c0; c < chunks; c += lanes) {
      T v[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        v[u] = from[u] ? *reinterpret_cast<const T*>(from[u] + c * kVec) : migrate_zero<T>();
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        const int64_t row = row0 + u * row_step;
        if (row < V_new) *reinterpret_cast<T*>(dst + row * ld_dst + c * kVec) = v[u];
      }
    }
  }
  if (bad) atomicOr(err, 1);
}

}  // namespace mapx

extern "C" int mapx_vocab_count_missing(const int64_t* keys, int64_t n, const int64_t* saved_table_keys,
                                        const int32_t* saved_table_rank, int64_t slot0, int64_t slots,
                                        int64_t n_slots_total, int64_t n_saved, int64_t* table_keys,
                                        int32_t* table_count, int32_t* table_first, int64_t capacity, int* err_flag,
                                        int64_t* missing_rows, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "vocab_count_missing: at most 2^31 - 1 rows");
  MAPX_REQUIRE(capacity >= 64 && (capacity & (capacity - 1)) == 0,
               "vocab_count_missing: capacity must be a power of two >= 64");
  MAPX_REQUIRE(n_saved >= 0 && slots >= 1 && (slots & (slots - 1)) == 0 && slots > n_saved && slot0 >= 0 &&
                   slot0 + slots <= n_slots_total,
               "vocab_count_missing: the saved field's slots must be a power of two, more than its keys, inside the table");
  MAPX_REQUIRE(err_flag && missing_rows, "vocab_count_missing: null pointer");
  MAPX_HIP(hipMemsetAsync(err_flag, 0, sizeof(int), stream));
  MAPX_HIP(hipMemsetAsync(missing_rows, 0, sizeof(int64_t), stream));
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(keys && table_keys && table_count && table_first && (n_saved == 0 || (saved_table_keys && saved_table_rank)),
               "vocab_count_missing: null pointer");
  hipLaunchKernelGGL(vocab_count_missing_kernel, dim3(grid_for(n, kGrowThreads, 8192)), dim3(kGrowThreads), 0, stream,
                     keys, n, saved_table_keys, saved_table_rank, slot0, slots, n_saved, table_keys, table_count,
                     table_first, capacity, err_flag, reinterpret_cast<unsigned long long*>(missing_rows));
  return check_launch("vocab_count_missing");
}

extern "C" int mapx_table_migrate(const float* src, int64_t ld_src, int64_t v_old, float* dst, int64_t ld_dst,
                                  int64_t v_new, int width, int n_fields, const int64_t* n_old, const int64_t* added,
                                  const int64_t* base_old, const int64_t* base_new, const float* fresh_opt,
                                  int64_t ld_fresh, int64_t n_fresh, int32_t* err, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n_fields >= 1 && n_fields <= MAPX_RT_MAX_FIELDS, "table_migrate: 1 to %d fields", MAPX_RT_MAX_FIELDS);
  MAPX_REQUIRE(width >= 1 && width <= 4096 && v_old >= 1 && v_new >= 0, "table_migrate: width in [1, 4096], v_old >= 1");
  MAPX_REQUIRE(ld_src >= width && ld_dst >= width, "table_migrate: a row pitch below the width");
  MAPX_REQUIRE(!fresh_opt || (ld_fresh >= width && n_fresh >= 0), "table_migrate: fresh needs ld_fresh >= width");
  MAPX_REQUIRE(err, "table_migrate: null pointer");
  MAPX_HIP(hipMemsetAsync(err, 0, sizeof(int32_t), stream));
  if (v_new == 0) return MAPX_OK;
  MAPX_REQUIRE(src && dst && n_old && added && base_old && base_new, "table_migrate: null pointer");
  auto aligned = [](const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; };
  const bool vec = width % 4 == 0 && aligned(src, ld_src) && aligned(dst, ld_dst) && (!fresh_opt || aligned(fresh_opt, ld_fresh));
  const int chunks = vec ? width / 4 : width;
  int log2_lanes = 0;
  while ((1 << log2_lanes) < chunks && log2_lanes < 6) ++log2_lanes;
  const int grid = grid_for(ceil_div(v_new, (int64_t)4) << log2_lanes, kGrowThreads);
  if (vec)
    hipLaunchKernelGGL(table_migrate_kernel<float4>, dim3(grid), dim3(kGrowThreads), 0, stream, src, ld_src, v_old, dst,
                       ld_dst, v_new, width, n_fields, n_old, added, base_old, base_new, fresh_opt, ld_fresh, n_fresh,
                       log2_lanes, err);
  else
    hipLaunchKernelGGL(table_migrate_kernel<float>, dim3(grid), dim3(kGrowThreads), 0, stream, src, ld_src, v_old, dst,
                       ld_dst, v_new, width, n_fields, n_old, added, base_old, base_new, fresh_opt, ld_fresh, n_fresh,
                       log2_lanes, err);
  return check_launch("table_migrate");
}
