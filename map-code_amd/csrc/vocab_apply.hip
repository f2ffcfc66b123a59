// A saved vocabulary applied to new rows: the reference's translation line
//   feat_map[key] if key in feat_map else feat_map[f'{name}-<oov>']      (proc_avazu.py:252-257, proc_criteo.py:155-160)
// against the feat_map of an earlier fit, for every field of a file in one launch.  Integer work, bit-exact.
//
// Tables.  The kept raw keys of all F fields lie concatenated in id order (keys [M], key_off [F+1]).  The ids of a
// feat_map are consecutive per field, so id = base_f + rank with rank = the key's position inside its field, and
// <oov>_f = base_f + n_f: only the rank is stored.  Field f owns the slots [tab_off[f], tab_off[f+1]) of two parallel
// arrays — key i64, rank i32: a 12-byte probe — a power of two of them and more than n_f, so a linear probe always
// meets an empty slot.  Slot = vocab_hash(key) & (slots_f - 1), as in the fit's table (vocab_hash.h).
//
//  load   clears the slots, then every key claims one (vocab_claim of vocab_hash.h, as vocab_count_kernel does) and
//         stores its rank.  Which slot a key of a collision chain gets depends on arrival; a lookup walks the chain
//         up to the first empty slot, so what it finds does not.
//  apply  a workgroup takes 64 rows x F fields at a time.  Wave w reads the 64 values of fields w, w+4, ... (a lane a
//         row: 512 contiguous bytes per load), probes the table with plain loads (it is constant during the launch)
//         and leaves rank | missing << 31 in an LDS tile [64][F | 1] (the odd pitch spreads a field's 64 rows over
//         the banks).  After a barrier the 256 threads sweep the tile row-major and store feat_ids / type_ids
//         contiguously along each row — F x 8 bytes per row, the whole tile one run when the pitch is F — instead of
//         one 8-byte store per 64-byte line and field.  OOV rows: ballot + popcount per wave and field into an LDS
//         counter that only that wave touches; one integer atomicAdd per workgroup and field at the end.
//         mode 1 stores every id straight from the probing lane, one 8-byte store per row and field F x 8 bytes
//         apart, for comparison.
// The fit translates its own column through the same two steps (mapx/vocab.py: build_field, build_vocab).
#include "../../include/mapx_hip.h"
#include "common.h"
#include "vocab_hash.h"

namespace mapx {

constexpr int kApplyRows = 64;                                   // rows of a tile = lanes of a wave
constexpr int kApplyThreads = 256;
constexpr int kApplyPitchMax = MAPX_RT_MAX_FIELDS | 1;

__global__ void __launch_bounds__(256) vocab_apply_clear_kernel(int64_t* __restrict__ tkey, int32_t* __restrict__ trank,
                                                                int64_t n_slots, int32_t* __restrict__ err) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    err[0] = 0;
    err[1] = INT32_MAX;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * blockDim.x) {
    tkey[i] = kVocabEmpty;
    trank[i] = -1;
  }
}

__device__ inline void vocab_apply_error(int32_t* __restrict__ err, int bit, int field) {
  atomicOr(err, bit);
  atomicMin(err + 1, field);
}

__global__ void __launch_bounds__(256) vocab_apply_load_kernel(const int64_t* __restrict__ keys,
                                                               const int64_t* __restrict__ key_off,
                                                               const int64_t* __restrict__ tab_off, int F, int64_t M,
                                                               int64_t n_slots, int64_t* __restrict__ tkey,
                                                               int32_t* __restrict__ trank, int32_t* __restrict__ err) {
  __shared__ int64_t s_koff[MAPX_RT_MAX_FIELDS + 1];
  for (int f = threadIdx.x; f <= F; f += blockDim.x) s_koff[f] = key_off[f];
  __syncthreads();
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = F;                                           // the field with key_off[f] <= j < key_off[f + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_koff[mid] <= j) lo = mid; else hi = mid;
    }
    const int f = lo;
    const int64_t t0 = tab_off[f], cap = tab_off[f + 1] - t0, nf = s_koff[f + 1] - s_koff[f];
    if (t0 < 0 || cap < 1 || (cap & (cap - 1)) != 0 || t0 + cap > n_slots || cap <= nf) {
      vocab_apply_error(err, 2, f);                               // no room for an empty slot: a probe could not end
      continue;
    }
    const int64_t k = keys[j];
    if (k == kVocabEmpty) {
      vocab_apply_error(err, 1, f);
      continue;
    }
    uint64_t s;
    switch (vocab_claim(tkey + t0, cap, k, &s)) {
      case kVocabClaimed: trank[t0 + s] = (int32_t)(j - s_koff[f]); break;
      case kVocabHeld: vocab_apply_error(err, 4, f); break;       // another position of this field holds the same key
      case kVocabFull: vocab_apply_error(err, 2, f); break;
    }
  }
}

template <bool DIRECT>
__global__ void __launch_bounds__(kApplyThreads) vocab_apply_kernel(
    const int64_t* const* __restrict__ cols, int64_t N, int F, const int64_t* __restrict__ tkey,
    const int32_t* __restrict__ trank, const int64_t* __restrict__ tab_off, int64_t n_slots,
    const int64_t* __restrict__ n_keys, const int64_t* __restrict__ base, const int64_t* __restrict__ flag,
    const int64_t* __restrict__ field_type, int64_t missing_type, int64_t* __restrict__ ids, int64_t ld_ids,
    int64_t* __restrict__ types, int64_t ld_types, unsigned long long* __restrict__ oov_rows,
    int32_t* __restrict__ err) {
  __shared__ uint32_t s_tile[DIRECT ? 1 : kApplyRows * kApplyPitchMax];
  __shared__ int64_t s_base[MAPX_RT_MAX_FIELDS], s_type[MAPX_RT_MAX_FIELDS];
  __shared__ unsigned long long s_oov[MAPX_RT_MAX_FIELDS];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, n_waves = kApplyThreads / kWave;
  const int pitch = F | 1;
  for (int f = threadIdx.x; f < F; f += kApplyThreads) {
    s_base[f] = base[f];
    s_type[f] = types ? field_type[f] : 0;
    s_oov[f] = 0;
  }
  __syncthreads();
  const int64_t n_tiles = ceil_div(N, (int64_t)kApplyRows);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row = tile * kApplyRows + lane;
    const bool live = row < N;
    for (int f = wave; f < F; f += n_waves) {                     // f is the same in every lane of the wave
      const int64_t v = live ? cols[f][row] : 0;
      const int64_t t0 = tab_off[f], cap = tab_off[f + 1] - t0, nf = n_keys[f];
      int32_t rank = (int32_t)nf;
      if (live) {
        if (v == kVocabEmpty) {
          vocab_apply_error(err, 1, f);
        } else if (nf > 0) {
          if (t0 < 0 || cap < 1 || (cap & (cap - 1)) != 0 || t0 + cap > n_slots)
            vocab_apply_error(err, 2, f);
          else
            rank = vocab_apply_probe(tkey, trank, t0, cap, nf, v);
        }
      }
      const unsigned long long oov = __ballot(live && rank == (int32_t)nf);
      if (lane == 0 && oov) s_oov[f] += (unsigned long long)__popcll(oov);   // wave f % 4 alone owns s_oov[f]
      const bool missing = types && flag[f] != 0 && v == -1;
      if (DIRECT) {
        if (live) {
          ids[row * ld_ids + f] = s_base[f] + rank;
          if (types) types[row * ld_types + f] = missing ? missing_type : s_type[f];
        }
      } else {
        s_tile[lane * pitch + f] = (uint32_t)rank | ((uint32_t)missing << 31);
      }
    }
    if (!DIRECT) {
      __syncthreads();
      const int64_t row0 = tile * kApplyRows;
      const int rows = (int)min((int64_t)kApplyRows, N - row0);
      for (int e = threadIdx.x; e < rows * F; e += kApplyThreads) {
        const int r = e / F, f = e - r * F;
        const uint32_t packed = s_tile[r * pitch + f];
        ids[(row0 + r) * ld_ids + f] = s_base[f] + (int64_t)(packed & 0x7fffffffu);
        if (types) types[(row0 + r) * ld_types + f] = (packed >> 31) ? missing_type : s_type[f];
      }
      __syncthreads();                                            // the tile is free for the next rows
    }
  }
  __syncthreads();
  for (int f = threadIdx.x; f < F; f += kApplyThreads)
    if (s_oov[f]) atomicAdd(oov_rows + f, s_oov[f]);
}

}  // namespace mapx

extern "C" size_t mapx_vocab_apply_table_slots(int64_t n_keys) {
  if (n_keys < 0 || n_keys >= ((int64_t)1 << 30)) return 0;
  size_t slots = 2;
  while ((int64_t)slots < 2 * n_keys) slots <<= 1;
  return slots;
}

extern "C" int mapx_vocab_apply_load(const int64_t* keys, const int64_t* key_off, const int64_t* tab_off, int n_fields,
                                     int64_t n_keys_total, int64_t n_slots_total, int64_t* table_keys,
                                     int32_t* table_rank, int32_t* err, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n_fields >= 1 && n_fields <= MAPX_RT_MAX_FIELDS, "vocab_apply_load: 1 to %d fields", MAPX_RT_MAX_FIELDS);
  MAPX_REQUIRE(n_keys_total >= 0 && n_slots_total >= n_fields, "vocab_apply_load: every field needs a slot");
  MAPX_REQUIRE(key_off && tab_off && table_keys && table_rank && err && (keys || n_keys_total == 0),
               "vocab_apply_load: null pointer");
  hipLaunchKernelGGL(vocab_apply_clear_kernel, dim3(grid_for(n_slots_total, 256)), dim3(256), 0, stream, table_keys,
                     table_rank, n_slots_total, err);
  if (int st = check_launch("vocab_apply_load (clear)")) return st;
  if (n_keys_total == 0) return MAPX_OK;
  hipLaunchKernelGGL(vocab_apply_load_kernel, dim3(grid_for(n_keys_total, 256, 8192)), dim3(256), 0, stream, keys,
                     key_off, tab_off, n_fields, n_keys_total, n_slots_total, table_keys, table_rank, err);
  return check_launch("vocab_apply_load");
}

extern "C" int mapx_vocab_apply(const int64_t* const* columns, int64_t n, int n_fields, const int64_t* table_keys,
                                const int32_t* table_rank, const int64_t* tab_off, int64_t n_slots_total,
                                const int64_t* n_keys, const int64_t* base, const int64_t* flag,
                                const int64_t* field_type, int64_t missing_type, int64_t* feat_ids, int64_t ld_ids,
                                int64_t* type_ids_opt, int64_t ld_types, int64_t* oov_rows, int32_t* err, int mode,
                                hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n_fields >= 1 && n_fields <= MAPX_RT_MAX_FIELDS, "vocab_apply: 1 to %d fields", MAPX_RT_MAX_FIELDS);
  MAPX_REQUIRE(n >= 0 && mode >= 0 && mode <= 1, "vocab_apply: n >= 0, mode 0 or 1");
  MAPX_REQUIRE(oov_rows && err, "vocab_apply: null pointer");
  MAPX_HIP(hipMemsetAsync(oov_rows, 0, (size_t)n_fields * sizeof(int64_t), stream));
  MAPX_HIP(hipMemsetAsync(err, 0, sizeof(int32_t), stream));
  MAPX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(err + 1), INT32_MAX, 1, stream));
  if (n == 0) return MAPX_OK;
  MAPX_REQUIRE(columns && table_keys && table_rank && tab_off && n_keys && base && feat_ids,
               "vocab_apply: null pointer");
  MAPX_REQUIRE(ld_ids >= n_fields, "vocab_apply: ld_ids must be at least the number of fields");
  MAPX_REQUIRE(!type_ids_opt || (flag && field_type && ld_types >= n_fields),
               "vocab_apply: type_ids need flag, field_type and ld_types >= the number of fields");
  const int grid = grid_for(ceil_div(n, (int64_t)kApplyRows), 1);
  unsigned long long* oov = reinterpret_cast<unsigned long long*>(oov_rows);
  if (mode == 0)
    hipLaunchKernelGGL(vocab_apply_kernel<false>, dim3(grid), dim3(kApplyThreads), 0, stream, columns, n, n_fields,
                       table_keys, table_rank, tab_off, n_slots_total, n_keys, base, flag, field_type, missing_type,
                       feat_ids, ld_ids, type_ids_opt, ld_types, oov, err);
  else
    hipLaunchKernelGGL(vocab_apply_kernel<true>, dim3(grid), dim3(kApplyThreads), 0, stream, columns, n, n_fields,
                       table_keys, table_rank, tab_off, n_slots_total, n_keys, base, flag, field_type, missing_type,
                       feat_ids, ld_ids, type_ids_opt, ld_types, oov, err);
  return check_launch("vocab_apply");
}
