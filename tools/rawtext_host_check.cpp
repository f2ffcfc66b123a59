// The line parser of csrc/rawtext_line.h on the CPU: the same text the parse kernel of csrc/rawtext.hip runs, over a
// heap buffer of exactly the file's size and an output of exactly rows x columns, so that a host sanitizer sees every
// byte the parser touches.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Iinclude tools/rawtext_host_check.cpp -o rawtext_host_check
//   ./rawtext_host_check avazu|criteo FILE
//
// Prints one line per data row, the output columns separated by blanks (the order of mapx.rawtext.Schema.columns), and
// returns 0; or prints `error line L column C reason R` (L: 1-based physical line, C: source column index, R:
// MAPX_RT_E_*) and returns 1.  Avazu's header line is compared with the schema's names and skipped.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../map-code_amd/csrc/rawtext_line.h"

namespace {

struct Reader {
  const uint8_t* p;
  uint32_t operator()(int32_t pos) const { return p[pos]; }
};

int64_t bucket_expr(int64_t v) {
  const double l = std::log((double)v);
  return (int64_t)std::floor(l * l);
}

// thresholds as mapx.rawtext.bucket_thresholds builds them: bisection on the expression itself
std::vector<int64_t> thresholds() {
  const int64_t top = INT64_MAX;
  std::vector<int64_t> t;
  for (int64_t b = 1; b <= bucket_expr(top); ++b) {
    int64_t lo = 3, hi = top;
    if (bucket_expr(lo) >= b) hi = lo;
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (bucket_expr(mid) >= b) hi = mid; else lo = mid;
    }
    t.push_back(hi);
  }
  return t;
}

const char* const kAvazuHeader =
    "id,click,hour,C1,banner_pos,site_id,site_domain,site_category,app_id,app_domain,app_category,device_id,device_ip,"
    "device_model,device_type,device_conn_type,C14,C15,C16,C17,C18,C19,C20,C21";

int add(mapx_rawtext_schema& s, int kind, int col) {
  s.kind[s.n_fields] = (uint8_t)kind;
  s.out_col[s.n_fields] = (int16_t)col;
  ++s.n_fields;
  return col + mapx::rt_kind_width(kind);
}

int build_schema(const std::string& name, mapx_rawtext_schema& s, bool& header) {
  memset(&s, 0, sizeof(s));
  int col = 0;
  if (name == "avazu") {
    s.delimiter = ',';
    header = true;
    col = add(s, MAPX_RT_SKIP, col);
    col = add(s, MAPX_RT_INT, col);
    col = add(s, MAPX_RT_YYMMDDHH, col);
    for (int f = 0; f < 2; ++f) col = add(s, MAPX_RT_INT, col);
    for (int f = 0; f < 9; ++f) col = add(s, MAPX_RT_HEX, col);
    for (int f = 0; f < 10; ++f) col = add(s, MAPX_RT_INT, col);
  } else if (name == "criteo") {
    s.delimiter = '\t';
    header = false;
    col = add(s, MAPX_RT_INT, col);
    for (int f = 0; f < 13; ++f) col = add(s, MAPX_RT_BUCKET, col);
    for (int f = 0; f < 26; ++f) col = add(s, MAPX_RT_HEX, col);
  } else {
    return -1;
  }
  return col;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s avazu|criteo FILE\n", argv[0]);
    return 2;
  }
  mapx_rawtext_schema schema;
  bool header = false;
  const int n_cols = build_schema(argv[1], schema, header);
  if (n_cols < 0) {
    fprintf(stderr, "unknown dataset %s\n", argv[1]);
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    perror(argv[2]);
    return 2;
  }
  std::vector<uint8_t> data;
  uint8_t block[65536];
  size_t got;
  while ((got = fread(block, 1, sizeof(block), f)) > 0) data.insert(data.end(), block, block + got);
  fclose(f);
  if (data.size() > ((size_t)1 << 30)) {
    fprintf(stderr, "at most 2^30 bytes\n");
    return 2;
  }
  std::vector<uint8_t> exact(data);                 // capacity == size: one byte too far is a heap overflow
  exact.shrink_to_fit();
  const int32_t n = (int32_t)exact.size();
  // the line index, by the rule of csrc/rawtext.hip: non-blank lines and their physical numbers
  std::vector<int32_t> line_start, line_no;
  int32_t no = 0;
  for (int32_t p = 0; p < n;) {
    int32_t e = p;
    while (e < n && exact[e] != '\n') ++e;
    int32_t len = e - p;
    if (len > 0 && exact[e - 1] == '\r') --len;
    if (len > 0) {
      line_start.push_back(p);
      line_no.push_back(no);
    }
    ++no;
    p = e + 1;
  }
  size_t first = 0;
  if (header) {
    if (line_start.empty()) {
      printf("error line 1 column 0 reason header\n");
      return 1;
    }
    int32_t e = line_start[0];
    while (e < n && exact[e] != '\n') ++e;
    if (e > line_start[0] && exact[e - 1] == '\r') --e;
    if (std::string(exact.begin() + line_start[0], exact.begin() + e) != kAvazuHeader) {
      printf("error line %d column 0 reason header\n", line_no[0] + 1);
      return 1;
    }
    first = 1;
  }
  const std::vector<int64_t> thr = thresholds();
  const int64_t rows = (int64_t)(line_start.size() - first);
  std::vector<int64_t> out((size_t)(rows * n_cols));
  uint64_t worst = ~(uint64_t)0;
  for (int64_t r = 0; r < rows; ++r) {
    int col = 0;
    const int reason = mapx::rt_parse_line(Reader{exact.data()}, line_start[first + r], n, &schema, thr.data(),
                                           (int)thr.size(), out.data(), rows, r, &col);
    if (reason) {
      const uint64_t w = mapx::rt_pack_error(line_no[first + r], col, reason);
      if (w < worst) worst = w;
    }
  }
  if (worst != ~(uint64_t)0) {
    printf("error line %u column %u reason %u\n", (unsigned)(worst >> 32) + 1, (unsigned)((worst >> 16) & 0xffff),
           (unsigned)(worst & 0xffff));
    return 1;
  }
  for (int64_t r = 0; r < rows; ++r) {
    for (int c = 0; c < n_cols; ++c) printf(c ? " %lld" : "%lld", (long long)out[(size_t)(c * rows + r)]);
    printf("\n");
  }
  return 0;
}
