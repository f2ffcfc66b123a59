// Raw delimited text -> device-resident int64 columns: read_feat of the reference's preprocessing
// (data_preprocess/proc_avazu.py:26-85: pandas per column over the gzipped CSV + a Python loop over datetimes;
// proc_criteo.py:24-88: pandas with dtype=object, one Python string per cell, then .map per column).
//
// One chunk of the file (cut at a line end by the host, <= 1 GiB so that offsets fit int32) lies in HBM as bytes.
//  (1) line index, three launches, integer only, no atomics:
//      count  per 16 KB tile {'\n' bytes, starts of non-blank lines}: 16-byte coalesced loads, the byte before and
//             after a lane's 16 come from the neighbour lanes (the wave's edge lanes load one byte each);
//      scan   exclusive prefix of the tile counts (one workgroup: <= 65 536 tiles);
//      fill   the count pass again with a workgroup scan: line_start / line_no of every non-blank line.
//  (2) parse: one lane per line, a wave (= a workgroup) owns 64 consecutive lines.  Their bytes are one contiguous
//      span: the wave copies it into LDS with 16-byte coalesced loads from a 16-byte aligned base and the lanes walk
//      their lines there (lane l's bytes lie ~one line length from lane l+1's: read from global memory every byte
//      load of the wave touches 64 cache lines).  A span larger than the window is read from global memory.  Both
//      run rt_parse_line (rawtext_line.h) over a byte reader; the schema table is a kernel argument copied to LDS.
// Reads stay below round_up(n_bytes, 16); bytes at or past n_bytes are never looked at as data.
#include "../../include/mapx_hip.h"
#include "common.h"
#include "rawtext_line.h"

namespace mapx {

constexpr int kRtTileBytes = 16384;              // 256 lanes x 16 bytes x 4 rounds
constexpr int kRtRounds = kRtTileBytes / (256 * 16);
constexpr int kRtWindow = 19456;                 // LDS window of one wave; with the schema 8 waves share a CU's 160 KB
constexpr int64_t kRtMaxBytes = (int64_t)1 << 30;

// The 16 bytes at offset o classified bit-parallel: nl = real '\n' bytes, st = bytes that start a non-blank line.
struct RtMasks {
  uint32_t nl, st;
};

__device__ inline uint32_t rt_eq_mask(const uint4& w, uint32_t byte) {
  const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) m |= (uint32_t)(((wd[i >> 2] >> ((i & 3) * 8)) & 0xffu) == byte) << i;
  return m;
}

// One round of a workgroup over the tile at `tile0`: lane `tid` owns bytes [o, o + 16).
__device__ inline RtMasks rt_classify(const uint8_t* __restrict__ buf, int64_t n, int64_t o) {
  const int lane = threadIdx.x & 63;
  const int64_t n16 = (n + 15) & ~(int64_t)15;
  uint4 w = make_uint4(0, 0, 0, 0);
  if (o < n16) w = *reinterpret_cast<const uint4*>(buf + o);
  // the byte before and the byte after, from the neighbour lanes; the wave's edge lanes read them themselves
  uint32_t prev = __shfl_up(w.w >> 24, 1, kWave);
  uint32_t next = __shfl_down(w.x & 0xffu, 1, kWave);
  if (lane == 0) prev = (o > 0 && o - 1 < n) ? buf[o - 1] : (uint32_t)'\n';
  if (lane == 63) next = (o + 16 < n) ? buf[o + 16] : (uint32_t)'\n';
  const int64_t left = n - o;
  const uint32_t inrange = left >= 16 ? 0xffffu : (left <= 0 ? 0u : ((1u << (int)left) - 1u));
  const uint32_t nl = rt_eq_mask(w, '\n') & inrange;
  const uint32_t cr = rt_eq_mask(w, '\r') & inrange;
  const uint32_t nlp = (nl | ~inrange) & 0xffffu;                     // past the end reads as '\n'
  const uint32_t next_nlp = (o + 16 >= n) || next == '\n';
  const uint32_t prev_nl = (o == 0) || prev == '\n';
  const uint32_t after_nl = ((nl << 1) | prev_nl) & 0xffffu;
  const uint32_t blank = nlp | (cr & ((nlp >> 1) | (next_nlp << 15)));
  return RtMasks{nl, after_nl & ~blank & inrange};
}

// tile_counts[t] = #'\n' | #starts << 16 (both <= 16 384)
__global__ void __launch_bounds__(256) rawtext_count_kernel(const uint8_t* __restrict__ buf, int64_t n,
                                                            uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t part[4];
  const int64_t tile0 = (int64_t)blockIdx.x * kRtTileBytes;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < kRtRounds; ++k) {
    const RtMasks m = rt_classify(buf, n, tile0 + k * 4096 + threadIdx.x * 16);
    c += __popc(m.nl) + ((uint32_t)__popc(m.st) << 16);
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// tile_offs[t] = {'\n' bytes before tile t, starts before tile t}; counts = the totals {starts, '\n' bytes}
__global__ void __launch_bounds__(1024) rawtext_scan_kernel(const uint32_t* __restrict__ tile_counts, int n_tiles,
                                                            int2* __restrict__ tile_offs, int32_t* __restrict__ counts) {
  __shared__ int s_nl[1024], s_st[1024];
  const int t = threadIdx.x;
  const int per = (n_tiles + 1023) / 1024;
  const int lo = min(t * per, n_tiles), hi = min(lo + per, n_tiles);
  int nl = 0, st = 0;
  for (int i = lo; i < hi; ++i) {
    const uint32_t c = tile_counts[i];
    nl += (int)(c & 0xffffu);
    st += (int)(c >> 16);
  }
  s_nl[t] = nl;
  s_st[t] = st;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {                                // inclusive Hillis-Steele over the 1024 ranges
    const int a = t >= d ? s_nl[t - d] : 0, b = t >= d ? s_st[t - d] : 0;
    __syncthreads();
    s_nl[t] += a;
    s_st[t] += b;
    __syncthreads();
  }
  int run_nl = s_nl[t] - nl, run_st = s_st[t] - st;
  for (int i = lo; i < hi; ++i) {
    const uint32_t c = tile_counts[i];
    tile_offs[i] = make_int2(run_nl, run_st);
    run_nl += (int)(c & 0xffffu);
    run_st += (int)(c >> 16);
  }
  if (t == 1023) {
    counts[0] = s_st[t];
    counts[1] = s_nl[t];
  }
}

__global__ void __launch_bounds__(256) rawtext_fill_kernel(const uint8_t* __restrict__ buf, int64_t n,
                                                           const int2* __restrict__ tile_offs,
                                                           int32_t* __restrict__ line_start,
                                                           int32_t* __restrict__ line_no, int64_t max_lines) {
  __shared__ uint32_t wave_sum[kRtRounds][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * kRtTileBytes;
  const int2 offs = tile_offs[blockIdx.x];
  RtMasks m[kRtRounds];
  uint32_t incl[kRtRounds];
#pragma unroll
  for (int k = 0; k < kRtRounds; ++k) {
    m[k] = rt_classify(buf, n, tile0 + k * 4096 + threadIdx.x * 16);
    uint32_t c = __popc(m[k].nl) + ((uint32_t)__popc(m[k].st) << 16);
    for (int o = 1; o < 64; o <<= 1) {                                // inclusive scan of the wave, byte order
      const uint32_t up = __shfl_up(c, o, kWave);
      if (lane >= o) c += up;
    }
    incl[k] = c;
    if (lane == 63) wave_sum[k][wave] = c;
  }
  __syncthreads();
  uint32_t base = 0;                                                  // packed counts of everything before this lane
#pragma unroll
  for (int k = 0; k < kRtRounds; ++k) {
    uint32_t before = base;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += wave_sum[k][w];
      base += wave_sum[k][w];
    }
    const uint32_t own = __popc(m[k].nl) + ((uint32_t)__popc(m[k].st) << 16);
    const uint32_t excl = before + incl[k] - own;
    const int nl0 = offs.x + (int)(excl & 0xffffu);
    int64_t idx = (int64_t)offs.y + (int64_t)(excl >> 16);
    const int64_t o = tile0 + k * 4096 + threadIdx.x * 16;
    uint32_t st = m[k].st;
    while (st) {
      const int i = __ffs(st) - 1;
      st &= st - 1;
      if (idx < max_lines) {
        line_start[idx] = (int32_t)(o + i);
        line_no[idx] = nl0 + __popc(m[k].nl & ((1u << i) - 1u));
      }
      ++idx;
    }
  }
}

struct RtGlobalReader {
  const uint8_t* p;
  __device__ uint32_t operator()(int32_t pos) const { return p[pos]; }
};
struct RtLdsReader {
  const uint8_t* p;                                                   // LDS, already offset by -span_lo
  int32_t lo;
  __device__ uint32_t operator()(int32_t pos) const { return p[pos - lo]; }
};

__global__ void __launch_bounds__(64) rawtext_parse_kernel(const uint8_t* __restrict__ buf, int32_t n,
                                                           const int32_t* __restrict__ line_start,
                                                           const int32_t* __restrict__ line_no, int32_t n_lines,
                                                           const mapx_rawtext_schema schema_arg,
                                                           const int64_t* __restrict__ thr, int n_thr,
                                                           int64_t* __restrict__ out, int64_t ld, int64_t row0,
                                                           unsigned long long* __restrict__ err, int mode) {
  __shared__ __attribute__((aligned(16))) uint8_t window[kRtWindow];
  __shared__ mapx_rawtext_schema schema;
  static_assert(sizeof(mapx_rawtext_schema) % 4 == 0, "schema is copied word by word");
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&schema_arg);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&schema);
    for (int i = threadIdx.x; i < (int)(sizeof(mapx_rawtext_schema) / 4); i += 64) dst[i] = src[i];
  }
  const int32_t first = (int32_t)blockIdx.x * 64;
  const int32_t line = first + (int32_t)threadIdx.x;
  const int32_t span_lo = line_start[first] & ~15;
  const int32_t span_end = first + 64 < n_lines ? line_start[first + 64] : n;
  const int32_t span_len = ((span_end + 15) & ~15) - span_lo;         // <= round_up(n, 16) - span_lo
  const bool staged = mode == 0 && span_len <= kRtWindow;
  if (staged) {
    for (int32_t o = (int32_t)threadIdx.x * 16; o < span_len; o += 64 * 16)
      *reinterpret_cast<uint4*>(window + o) = *reinterpret_cast<const uint4*>(buf + span_lo + o);
  }
  __syncthreads();
  if (line >= n_lines) return;
  const int32_t pos = line_start[line];
  int col = 0, reason;
  if (staged)
    reason = rt_parse_line(RtLdsReader{window, span_lo}, pos, n, &schema, thr, n_thr, out, ld, row0 + line, &col);
  else
    reason = rt_parse_line(RtGlobalReader{buf}, pos, n, &schema, thr, n_thr, out, ld, row0 + line, &col);
  if (reason) atomicMin(err, (unsigned long long)rt_pack_error(line_no[line], col, reason));
}

inline int rt_tiles(int64_t n_bytes) { return (int)ceil_div(n_bytes, kRtTileBytes); }
inline size_t rt_counts_bytes(int64_t n_bytes) { return ((size_t)rt_tiles(n_bytes) * 4 + 15) & ~(size_t)15; }

}  // namespace mapx

extern "C" size_t mapx_rawtext_index_workspace_bytes(int64_t n_bytes) {
  using namespace mapx;
  if (n_bytes < 0 || n_bytes > kRtMaxBytes) return 0;
  return rt_counts_bytes(n_bytes) + (size_t)rt_tiles(n_bytes) * sizeof(int2) + 16;
}

extern "C" int mapx_rawtext_index(const uint8_t* buf, int64_t n_bytes, void* workspace, size_t workspace_bytes,
                                  int32_t* line_start, int32_t* line_no, int64_t max_lines, int32_t* counts,
                                  hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(n_bytes >= 0 && n_bytes <= kRtMaxBytes, "rawtext_index: a chunk holds at most 2^30 bytes");
  MAPX_REQUIRE(counts && max_lines >= 0, "rawtext_index: bad arguments");
  if (n_bytes == 0) {
    MAPX_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), stream));
    return MAPX_OK;
  }
  MAPX_REQUIRE(buf && ((uintptr_t)buf & 15) == 0, "rawtext_index: buf must be 16-byte aligned");
  MAPX_REQUIRE(max_lines == 0 || (line_start && line_no), "rawtext_index: null pointer");
  MAPX_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "rawtext_index: workspace must be 16-byte aligned");
  if (workspace_bytes < mapx_rawtext_index_workspace_bytes(n_bytes)) {
    set_error("rawtext_index: workspace of %zu bytes, %zu needed", workspace_bytes,
              mapx_rawtext_index_workspace_bytes(n_bytes));
    return MAPX_EWORKSPACE;
  }
  const int tiles = rt_tiles(n_bytes);
  uint32_t* tile_counts = reinterpret_cast<uint32_t*>(workspace);
  int2* tile_offs = reinterpret_cast<int2*>(reinterpret_cast<char*>(workspace) + rt_counts_bytes(n_bytes));
  hipLaunchKernelGGL(rawtext_count_kernel, dim3(tiles), dim3(256), 0, stream, buf, n_bytes, tile_counts);
  hipLaunchKernelGGL(rawtext_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_counts, tiles, tile_offs, counts);
  hipLaunchKernelGGL(rawtext_fill_kernel, dim3(tiles), dim3(256), 0, stream, buf, n_bytes, tile_offs, line_start,
                     line_no, max_lines);
  return check_launch("rawtext_index");
}

extern "C" int mapx_rawtext_parse(const uint8_t* buf, int64_t n_bytes, const int32_t* line_start,
                                  const int32_t* line_no, int64_t n_lines, const mapx_rawtext_schema* schema,
                                  const int64_t* thresholds, int n_thresholds, int64_t* out, int64_t ld, int64_t row0,
                                  int n_cols, uint64_t* err, int mode, hipStream_t stream) {
  using namespace mapx;
  MAPX_REQUIRE(err && schema, "rawtext_parse: null pointer");
  MAPX_REQUIRE(mode == 0 || mode == 1, "rawtext_parse: mode is 0 (automatic) or 1 (direct)");
  MAPX_REQUIRE(n_bytes >= 0 && n_bytes <= kRtMaxBytes, "rawtext_parse: a chunk holds at most 2^30 bytes");
  MAPX_REQUIRE(n_lines >= 0 && n_lines <= n_bytes, "rawtext_parse: more lines than bytes");
  MAPX_REQUIRE(schema->n_fields >= 1 && schema->n_fields <= MAPX_RT_MAX_FIELDS && schema->delimiter > 0 &&
                   schema->delimiter < 256 && schema->delimiter != '\n' && schema->delimiter != '\r' &&
                   schema->delimiter != '"',
               "rawtext_parse: bad schema header");
  bool buckets = false;
  for (int f = 0; f < schema->n_fields; ++f) {
    const int kind = schema->kind[f];
    MAPX_REQUIRE(kind >= MAPX_RT_SKIP && kind <= MAPX_RT_YYMMDDHH, "rawtext_parse: field %d has unknown kind %d", f, kind);
    MAPX_REQUIRE(kind == MAPX_RT_SKIP || (schema->out_col[f] >= 0 && schema->out_col[f] + rt_kind_width(kind) <= n_cols),
                 "rawtext_parse: field %d writes outside the %d output columns", f, n_cols);
    buckets |= kind == MAPX_RT_BUCKET;
  }
  MAPX_REQUIRE(!buckets || (thresholds && n_thresholds >= 1), "rawtext_parse: BUCKET fields need the threshold table");
  MAPX_REQUIRE(n_thresholds >= 0, "rawtext_parse: negative table size");
  MAPX_HIP(hipMemsetAsync(err, 0xff, sizeof(uint64_t), stream));
  if (n_lines == 0) return MAPX_OK;
  MAPX_REQUIRE(buf && ((uintptr_t)buf & 15) == 0, "rawtext_parse: buf must be 16-byte aligned");
  MAPX_REQUIRE(line_start && line_no && out, "rawtext_parse: null pointer");
  MAPX_REQUIRE(row0 >= 0 && ld >= row0 + n_lines, "rawtext_parse: column pitch %lld < row offset + lines",
               (long long)ld);
  hipLaunchKernelGGL(rawtext_parse_kernel, dim3((unsigned)ceil_div(n_lines, 64)), dim3(64), 0, stream, buf,
                     (int32_t)n_bytes, line_start, line_no, (int32_t)n_lines, *schema, thresholds, n_thresholds, out, ld,
                     row0, reinterpret_cast<unsigned long long*>(err), mode);
  return check_launch("rawtext_parse");
}

extern "C" int mapx_rawtext_window_bytes(void) { return mapx::kRtWindow; }
