// One line of delimited raw text -> its int64 output columns: the tokenizer and the field grammars of
// csrc/rawtext.hip (read_feat of data_preprocess/proc_avazu.py:26-85 and proc_criteo.py:24-88).
//
// The same text runs on the device (hipcc) and on the CPU (any C++17 compiler: tools/rawtext_host_check.cpp), so
// every byte access of the parser can be put under a host sanitizer.  Nothing here touches memory except through
// the byte reader `rd(pos)` (pos in [0, n_bytes)), the schema, the threshold table and the output columns.
//
// A line starts at `pos` and ends at the first '\n' at or after it, or at n_bytes; one '\r' directly in front of
// that end is not part of the line.  Fields are separated by the schema's delimiter byte; there is no quoting: a
// '"' anywhere in the line is an error.  Grammar per kind (stricter than Python's int(): no '+', no blanks, no '_'):
//   SKIP      anything                                   writes nothing
//   INT       -?[0-9]{1,18}                              the value
//   BUCKET    empty -> -1, else INT syntax               v <= 2 -> v, else #{thresholds <= v} = floor(log(v)^2)
//   HEX       empty -> -1, else [0-9a-f]{1,14}           (value << 4) | width
//   YYMMDDHH  8 digits of a valid date and hour          weekday (Monday = 0), day, hour, weekday > 4
#pragma once
#include <stdint.h>

#include "../../include/mapx_hip.h"

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ inline
#else
#define RT_HD inline
#endif

namespace mapx {

// (line, source column, reason) of an error as one word: an integer min over the words of all bad lines picks the
// smallest physical line, then the smallest column.
RT_HD uint64_t rt_pack_error(int32_t line_no, int col, int reason) {
  return ((uint64_t)(uint32_t)line_no << 32) | ((uint64_t)(uint32_t)(col & 0xffff) << 16) | (uint64_t)(uint32_t)reason;
}

RT_HD int rt_kind_width(int kind) {
  return kind == MAPX_RT_SKIP ? 0 : (kind == MAPX_RT_YYMMDDHH ? 4 : 1);
}

// floor(log(v)^2) for v > 2 without a logarithm: thr[b-1] is the smallest v whose bucket is >= b.
RT_HD int64_t rt_bucket(int64_t v, const int64_t* thr, int n_thr) {
  int lo = 0, hi = n_thr;                       // number of thresholds <= v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Days since 1970-01-01 of a proleptic Gregorian date (H. Hinnant's days_from_civil; integer only).
RT_HD int32_t rt_days_from_civil(int32_t y, int32_t m, int32_t d) {
  y -= m <= 2;
  const int32_t era = (y >= 0 ? y : y - 399) / 400;
  const int32_t yoe = y - era * 400;
  const int32_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

RT_HD int rt_days_in_month(int32_t y, int32_t m) {
  const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
  return m == 2 ? (leap ? 29 : 28) : ((m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31);
}

// Parses the line at `pos` and writes its values to out[(column) * ld + row].  -> 0, or the reason with *err_col
// = the source column.  A bad line stops at its first bad field: what it wrote before stays inside row `row`.
template <class Reader>
RT_HD int rt_parse_line(const Reader& rd, int32_t pos, int32_t n_bytes, const mapx_rawtext_schema* s,
                        const int64_t* thr, int n_thr, int64_t* out, int64_t ld, int64_t row, int* err_col) {
  const uint32_t delim = (uint32_t)s->delimiter;
  const int nf = s->n_fields;
  for (int f = 0; f < nf; ++f) {
    const int kind = s->kind[f];
    uint64_t v = 0;
    int nch = 0, ndig = 0;
    bool neg = false, bad = false, eol;
    *err_col = f;
    for (;;) {
      const uint32_t c = pos < n_bytes ? rd(pos) : (uint32_t)'\n';
      eol = c == '\n' || (c == '\r' && (pos + 1 >= n_bytes || rd(pos + 1) == '\n'));
      if (eol || c == delim) break;
      if (c == '"') return MAPX_RT_E_QUOTE;
      const uint32_t d = c - '0';
      if (kind == MAPX_RT_HEX) {
        const uint32_t x = c - 'a';
        if (d <= 9) { v = (v << 4) | d; ++ndig; }
        else if (x <= 5) { v = (v << 4) | (x + 10); ++ndig; }
        else bad = true;
      } else if (kind != MAPX_RT_SKIP) {
        if (d <= 9) { v = v * 10 + d; ++ndig; }
        else if (c == '-' && nch == 0 && kind != MAPX_RT_YYMMDDHH) neg = true;
        else bad = true;
      }
      ++nch;
      ++pos;
    }
    int64_t* o = out + (int64_t)s->out_col[f] * ld + row;
    if (kind == MAPX_RT_INT || kind == MAPX_RT_BUCKET) {
      if (kind == MAPX_RT_BUCKET && nch == 0) {
        *o = -1;
      } else {
        if (bad || ndig < 1 || ndig > 18) return MAPX_RT_E_INT;
        const int64_t x = neg ? -(int64_t)v : (int64_t)v;
        *o = (kind == MAPX_RT_BUCKET && x > 2) ? rt_bucket(x, thr, n_thr) : x;
      }
    } else if (kind == MAPX_RT_HEX) {
      if (nch == 0) {
        *o = -1;
      } else {
        if (bad || ndig > 14) return MAPX_RT_E_HEX;
        *o = (int64_t)((v << 4) | (uint64_t)ndig);
      }
    } else if (kind == MAPX_RT_YYMMDDHH) {
      if (bad || ndig != 8) return MAPX_RT_E_DATE;
      const int32_t w = (int32_t)v;
      const int32_t yy = w / 1000000, mm = w / 10000 % 100, dd = w / 100 % 100, hh = w % 100;
      const int32_t year = yy <= 68 ? 2000 + yy : 1900 + yy;           // strptime's %y
      if (mm < 1 || mm > 12 || dd < 1 || dd > rt_days_in_month(year, mm) || hh > 23) return MAPX_RT_E_DATE;
      const int32_t days = rt_days_from_civil(year, mm, dd);
      const int32_t wd = ((days + 3) % 7 + 7) % 7;                     // 1970-01-01 was a Thursday
      o[0] = wd;
      o[ld] = dd;
      o[2 * ld] = hh;
      o[3 * ld] = wd > 4;
    }
    if (f + 1 < nf) {
      if (eol) { *err_col = f + 1; return MAPX_RT_E_FEW; }
      ++pos;                                                            // the delimiter
    } else if (!eol) {
      return MAPX_RT_E_MANY;
    }
  }
  return 0;
}

}  // namespace mapx
