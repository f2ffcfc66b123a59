// Scoring (mapx/score.py): the two launches a scoring step has beyond the model's forward.  Both walk an id matrix /
// an output vector of N rows by a device-side cursor, so that a captured step (block -> forward -> sink -> advance)
// replays on the next B rows without a host write in between (mapx_step_advance moves the cursor).
//
//   score_block  batch[i, :] = ids[c + i, :] for c + i < N, zeros (<pad>) behind the end;  oov_fields[c + i] = the
//                number of fields of the row that hold their field's <oov> id.
//   score_sink   logits_out[c + i] = logits[i], probs[c + i] = sigmoid(logits[i]) (fp32, THE sigmoid of metrics.hip),
//                rows behind the end dropped.
//
// Streaming kernels: 16-byte accesses along rows wherever the addresses allow, 8 / 4-byte ones otherwise; no atomics;
// 64-bit row numbers.  HBM traffic: block B F 16 + B bytes, sink B 12 bytes.
#include "../../include/mapx_hip.h"
#include "common.h"

namespace mapx {

typedef long long i64x2_t __attribute__((ext_vector_type(2)));

constexpr int kScoreBlock = 256;

// G lanes per row (a power of two >= (F + 1) / 2).  Lane j of a row's group owns the columns {2j - s, 2j - s + 1} with
// s = the parity of the row's offset i F inside `batch`: its pair then starts at an even element of `batch`, whose
// base is 16-byte aligned, so every store of two valid columns is one 16-byte store (an odd F shifts every other row
// by one element).  The load of the pair is one 16-byte load when its source address is even too.
template <int G>
__global__ void __launch_bounds__(kScoreBlock) score_block_kernel(const int64_t* __restrict__ ids, int64_t ld, int64_t N,
                                                                  const int64_t* __restrict__ cursor, int64_t B, int F,
                                                                  const int64_t* __restrict__ oov_id,
                                                                  int64_t* __restrict__ batch,
                                                                  uint8_t* __restrict__ oov_fields) {
  constexpr int kRows = kScoreBlock / G;
  const int64_t c0 = *cursor;
  const int j = threadIdx.x % G;
  const bool ids_even = (reinterpret_cast<uintptr_t>(ids) & 15) == 0;
  for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / G; i < B; i += (int64_t)gridDim.x * kRows) {
    const int64_t r = c0 + i;
    const bool live = r >= 0 && r < N;
    const int64_t o = i * F;                         // the row's offset inside batch
    const int c = 2 * j - (int)(o & 1);              // first column of this lane's pair
    const bool has0 = c >= 0 && c < F, has1 = c + 1 >= 0 && c + 1 < F;
    int64_t v0 = 0, v1 = 0;
    int hits = 0;
    if (live) {
      const int64_t s = r * ld + c;                  // source element of column c
      if (has0 && has1 && ids_even && (s & 1) == 0) {
        const i64x2_t v = *reinterpret_cast<const i64x2_t*>(ids + s);
        v0 = v[0];
        v1 = v[1];
      } else {
        if (has0) v0 = ids[s];
        if (has1) v1 = ids[s + 1];
      }
      hits = (int)(has0 && v0 == oov_id[has0 ? c : 0]) + (int)(has1 && v1 == oov_id[has1 ? c + 1 : 0]);
    }
    if (has0 && has1) {
      i64x2_t v;
      v[0] = v0;
      v[1] = v1;
      *reinterpret_cast<i64x2_t*>(batch + o + c) = v;
    } else if (has0) {
      batch[o + c] = v0;
    } else if (has1) {
      batch[o + c + 1] = v1;
    }
    hits = group_sum<G, int>(hits);                  // (every lane of the group is here: the loop bound is per row)
    if (live && j == 0) oov_fields[r] = (uint8_t)hits;
  }
}

// Four consecutive rows per thread: one 16-byte load of the logits and 16-byte stores when the four destinations lie
// inside N and start at a multiple of four elements, all three bases being 16-byte aligned; single elements otherwise.
__global__ void __launch_bounds__(kScoreBlock) score_sink_kernel(const float* __restrict__ logits, int64_t N,
                                                                 const int64_t* __restrict__ cursor, int64_t B,
                                                                 float* __restrict__ probs,
                                                                 float* __restrict__ logits_out) {
  const int64_t c0 = *cursor;
  const bool even = ((reinterpret_cast<uintptr_t>(probs) | reinterpret_cast<uintptr_t>(logits_out) |
                      reinterpret_cast<uintptr_t>(logits)) & 15) == 0;
  const int64_t quads = ceil_div(B, 4);
  for (int64_t q = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kScoreBlock) {
    const int64_t i = 4 * q, r = c0 + i;
    if (r >= N || r + 3 < 0) continue;
    if (i + 3 < B && r >= 0 && r + 3 < N && even && (r & 3) == 0) {
      const float4 x = load4(logits + i);
      store4(logits_out + r, x);
      store4(probs + r, make_float4(sigmoid_f32(x.x), sigmoid_f32(x.y), sigmoid_f32(x.z), sigmoid_f32(x.w)));
    } else {
      for (int k = 0; k < 4; ++k) {
        if (i + k >= B || r + k < 0 || r + k >= N) continue;
        const float x = logits[i + k];
        logits_out[r + k] = x;
        probs[r + k] = sigmoid_f32(x);
      }
    }
  }
}

}  // namespace mapx

extern "C" int mapx_score_block(const int64_t* ids, int64_t ld_ids, int64_t N, const int64_t* cursor, int64_t B, int F,
                                const int64_t* oov_id, int64_t* batch, uint8_t* oov_fields, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(cursor && oov_id && batch && B >= 0 && N >= 0, "score_block: bad arguments");
  MAPX_REQUIRE(F >= 1 && F <= 64, "score_block: 1 <= F <= 64 (F = %d)", F);
  MAPX_REQUIRE(N == 0 || (ids && oov_fields && ld_ids >= F), "score_block: N rows need ids at a pitch >= F and oov_fields");
  MAPX_REQUIRE((reinterpret_cast<uintptr_t>(batch) & 15) == 0, "score_block: batch must be 16-byte aligned");
  if (B == 0) return MAPX_OK;
  const int need = (F + 1) / 2;
  int G = 1;
  while (G < need) G *= 2;
  const int grid = grid_for(B, kScoreBlock / G);
#define MAPX_SCORE_BLOCK(g)                                                                                        \
  case g:                                                                                                          \
    hipLaunchKernelGGL(score_block_kernel<g>, dim3(grid), dim3(kScoreBlock), 0, stream, ids, ld_ids, N, cursor, B, \
                       F, oov_id, batch, oov_fields);                                                              \
    break;
  switch (G) {
    MAPX_SCORE_BLOCK(1)
    MAPX_SCORE_BLOCK(2)
    MAPX_SCORE_BLOCK(4)
    MAPX_SCORE_BLOCK(8)
    MAPX_SCORE_BLOCK(16)
    MAPX_SCORE_BLOCK(32)
  }
#undef MAPX_SCORE_BLOCK
  return check_launch("score_block");
}

extern "C" int mapx_score_sink(const float* logits, int64_t N, const int64_t* cursor, int64_t B, float* probs,
                               float* logits_out, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(cursor && B >= 0 && N >= 0, "score_sink: bad arguments");
  MAPX_REQUIRE(B == 0 || logits, "score_sink: B logits");
  MAPX_REQUIRE(N == 0 || (probs && logits_out), "score_sink: N rows need probs and logits_out");
  if (B == 0 || N == 0) return MAPX_OK;
  hipLaunchKernelGGL(score_sink_kernel, dim3(grid_for(ceil_div(B, 4), kScoreBlock)), dim3(kScoreBlock), 0, stream, logits,
                     N, cursor, B, probs, logits_out);
  return check_launch("score_sink");
}
