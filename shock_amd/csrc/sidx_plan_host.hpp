// sidx_plan_host.hpp -- the host arithmetic of the index read path and of the download plan
// (shockidx_download_plan): the part strings (strconv.ParseInt, strings.Split on '-'), the
// virtual size index (index/virtual.go:50-80) and the order in which a request's errors are
// reported (controller/node/single.go:372-483 handles the parts in order and fails at the first
// error).  No HIP types: tests/host/plan_test.cpp builds it alone under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#ifdef __HIP__
#define SIDX_PLAN_HD __host__ __device__  // chunk_segment: the level-2 kernel runs the same lines
#else
#define SIDX_PLAN_HD
#endif

namespace sidx_plan {

typedef unsigned long long u64;  // (sidx_common.hpp's, which needs HIP)
typedef long long i64;

const char E_IDX_RANGE[] = "Invalid index record range";  // errors/errors.go:21-23
const char E_IDX_BOUNDS[] = "Index record out of bounds";
const char E_IDX_NOFILE[] = "Index file is missing";

constexpr u64 MAX_PARTS = 1ull << 20;        // parts of one plan
constexpr u64 MAX_VISITS = (u64)INT32_MAX;  // rows one level of a plan may visit

// strconv.ParseInt(s, 10, 64); any error (syntax or range) is reported the same by the callers
inline bool go_parse_int64(const char *s, size_t n, i64 *v) {
  size_t i = 0;
  bool neg = false;
  if (n == 0) return false;
  if (s[0] == '+' || s[0] == '-') {
    neg = s[0] == '-';
    i = 1;
  }
  if (i == n) return false;
  u64 u = 0;
  for (; i < n; ++i) {
    const unsigned d = (unsigned char)s[i] - '0';
    if (d > 9 || u > (~0ull - d) / 10) return false;
    u = u * 10 + d;
  }
  if (!neg && u > (u64)INT64_MAX) return false;
  if (neg && u > (u64)INT64_MAX + 1) return false;
  *v = neg ? (i64)(0 - u) : (i64)u;
  return true;
}

// the two fields of "start-end" (strings.Split(part, "-")[0], [1]; further fields are ignored)
inline bool split_range(const char *part, const char *dash, i64 *start, i64 *end) {
  const char *s1 = dash + 1, *d2 = strchr(s1, '-');
  const bool ok0 = go_parse_int64(part, (size_t)(dash - part), start);
  const bool ok1 = go_parse_int64(s1, d2 ? (size_t)(d2 - s1) : strlen(s1), end);
  return ok0 && ok1;
}

// the part string: 0 = one record, 1 = a range start-end, -1 = Go's error text in *e
inline int parse_part(const char *part, i64 idx_length, i64 *a, i64 *b, const char **e) {
  const char *dash = strchr(part, '-');
  if (dash) {  // index.go:77-84 / :129-136
    i64 start = 0, end = 0;
    if (!split_range(part, dash, &start, &end) || start <= 0 || start > idx_length || end <= 0 || end > idx_length) {
      *e = E_IDX_RANGE;
      return -1;
    }
    *a = start;
    *b = end;
    return 1;
  }
  i64 p = 0;  // index.go:100-105 / :178-183
  if (!go_parse_int64(part, strlen(part), &p) || p <= 0 || p > idx_length) {
    *e = E_IDX_BOUNDS;
    return -1;
  }
  *a = *b = p;
  return 0;
}

// rows Idx.Range visits for a parsed part: one record ("N", "N-N") reads one row, b < a none
// (the coalescing loop runs zero times), else rows a-1 .. b-1
inline u64 range_visits(int kind, i64 a, i64 b) {
  if (kind == 0 || a == b) return 1;
  return b < a ? 0 : (u64)(b - a) + 1;
}

// SizePart (virtual.go:50-80) in wrapping int64: the products and sums are taken mod 2^64 and
// compared as int64, like Go's.  0 and *pos, *len, or -1 and Go's error text in *e.
inline int size_part(const char *part, i64 size, i64 chunk, i64 *pos, i64 *len, const char **e) {
  typedef u64 u;
  const auto mul = [](i64 x, i64 y) { return (i64)((u)x * (u)y); };
  const auto add = [](i64 x, i64 y) { return (i64)((u)x + (u)y); };
  const auto sub = [](i64 x, i64 y) { return (i64)((u)x - (u)y); };
  const char *dash = strchr(part, '-');
  if (dash) {  // :51-65
    i64 start = 0, end = 0;
    if (!split_range(part, dash, &start, &end) || start <= 0 || mul(start - 1, chunk) > size || end <= 0 ||
        mul(end - 1, chunk) > size) {
      *e = E_IDX_RANGE;
      return -1;
    }
    *pos = mul(start - 1, chunk);
    const i64 full = sub(mul(end - 1, chunk), mul(start - 1, chunk));
    if (add(add(full, chunk), *pos) > size) *len = add(full, sub(size, add(*pos, full)));
    else *len = add(full, chunk);
    return 0;
  }
  i64 p = 0;  // :66-78
  if (!go_parse_int64(part, strlen(part), &p) || p <= 0 || mul(p - 1, chunk) > size) {
    *e = E_IDX_BOUNDS;
    return -1;
  }
  *pos = mul(p - 1, chunk);
  *len = sub(size, *pos) < chunk ? sub(size, *pos) : chunk;
  return 0;
}

// One part of a plan as the device sees it: rows a0 .. a0 + nr - 1 of the index (Range), or rows
// a0 and b0 (Part, kind 1) / row a0 alone (Part, kind 0).
struct Seg {
  u64 a0, b0, nr;
  int kind;
};

// The parts of a request up to its first parse or bounds error.
struct Parsed {
  std::vector<Seg> segs;      // parts 0 .. segs.size() - 1 parsed
  i64 err_part = -1;      // the first part that did not (== segs.size()), -1: none
  const char *err = nullptr;  //   Go's text for it
  u64 visits = 0;        // rows a Range plan of segs visits (the sum of nr; above MAX_VISITS: too many)
  i64 first_nonempty = -1;  // the first part with nr > 0: where a level 2 is first reached
};
inline Parsed parse_parts(const char *const *parts, u64 nparts, i64 idx_length) {
  Parsed out;
  out.segs.reserve(nparts);
  for (u64 k = 0; k < nparts; ++k) {
    i64 a = 0, b = 0;
    const int kind = parse_part(parts[k], idx_length, &a, &b, &out.err);
    if (kind < 0) {
      out.err_part = (i64)k;
      break;
    }
    const Seg s = {(u64)(a - 1), (u64)(b - 1), range_visits(kind, a, b), kind};
    if (s.nr && out.first_nonempty < 0) out.first_nonempty = (i64)k;
    out.visits += s.nr > MAX_VISITS ? MAX_VISITS + 1 : s.nr;  // (saturating: the sum cannot wrap)
    out.segs.push_back(s);
  }
  return out;
}

// A level-2 segment of CHUNK_RANGE (single.go:411-414): the matrix record (c0, c1) as the record
// range "start-stop".  Invalid (Go's InvalidIndexRange from recordIdx.Range) when either is <= 0
// or above rec_length; a negative value formats with a leading '-', which strings.Split turns into
// an empty field and ParseInt into an error -- the same text.  Else *a0 = start - 1 and *nr rows.
SIDX_PLAN_HD inline bool chunk_segment(i64 c0, i64 c1, i64 rec_length, u64 *a0, u64 *nr) {
  const i64 start = c0 / 16 + 1;
  const i64 stop = (i64)((u64)(start - 1) + (u64)(c1 / 16));
  *a0 = 0;
  *nr = 0;
  if (start <= 0 || start > rec_length || stop <= 0 || stop > rec_length) return false;
  *a0 = (u64)(start - 1);
  *nr = stop < start ? 0 : (u64)(stop - start) + 1;
  return true;
}

// The error of a request, by Go's order of evaluation.  Parts are handled in order; within part k
// its own parse or bounds error (parse_part) comes before anything its level 2 does, and both come
// after every error of a part before k.
//   l2_key:      the smallest (part << 32 | record-in-request) of an invalid level-2 segment among
//                the parts before the parse error, ~0: none
//   nofile_part: the first part whose level 1 yields a record while the record index is missing
//                (recordIdx.Range fails at os.Open, before it parses), -1: none
struct PlanError {
  i64 part = -1;
  const char *text = nullptr;
};
inline PlanError first_error(const Parsed &p, u64 l2_key, i64 nofile_part) {
  PlanError e;
  if (nofile_part >= 0) {  // (always before p.err_part: only parsed parts reach level 2)
    e.part = nofile_part;
    e.text = E_IDX_NOFILE;
  } else if (l2_key != ~0ull) {
    e.part = (i64)(l2_key >> 32);
    e.text = E_IDX_RANGE;
  } else if (p.err_part >= 0) {
    e.part = p.err_part;
    e.text = p.err;
  }
  return e;
}

}  // namespace sidx_plan
