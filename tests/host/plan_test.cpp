// plan_test.cpp -- CPU test of the download plan's host arithmetic in
// shock_amd/csrc/sidx_plan_host.hpp: the part strings (strconv.ParseInt, strings.Split), SizePart
// in wrapping int64 (index/virtual.go:50-80), the level-2 segment of a matrix record
// (controller/node/single.go:412-414) and the order in which a request's errors are reported.
// Stand-alone: it includes that header only, links nothing of the library and makes no HIP call.
// Built with the host sanitizers by `make -C shock_amd/csrc plan_test` (a signed overflow would be
// a UBSan report); exit 0 = every check held.  The expected values are read off the Go lines cited.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "sidx_plan_host.hpp"

using namespace sidx_plan;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static const i64 I64_MIN = INT64_MIN, I64_MAX = INT64_MAX;

static void test_parse_int() {
  i64 v = 7;
  CHECK(go_parse_int64("0", 1, &v) && v == 0);
  CHECK(go_parse_int64("+12", 3, &v) && v == 12);
  CHECK(go_parse_int64("-12", 3, &v) && v == -12);
  CHECK(go_parse_int64("9223372036854775807", 19, &v) && v == I64_MAX);
  CHECK(go_parse_int64("-9223372036854775808", 20, &v) && v == I64_MIN);
  CHECK(!go_parse_int64("9223372036854775808", 19, &v));   // value out of range
  CHECK(!go_parse_int64("-9223372036854775809", 20, &v));
  CHECK(!go_parse_int64("99999999999999999999", 20, &v));  // past uint64 too
  CHECK(!go_parse_int64("", 0, &v) && !go_parse_int64("-", 1, &v) && !go_parse_int64("+", 1, &v));
  CHECK(!go_parse_int64("1 ", 2, &v) && !go_parse_int64("0x1", 3, &v) && !go_parse_int64("1_0", 3, &v));
  CHECK(go_parse_int64("12-3", 2, &v) && v == 12);  // length-bounded: a field of a longer string
}

static void test_parse_part() {
  i64 a = 0, b = 0;
  const char *e = nullptr;
  CHECK(parse_part("3", 6, &a, &b, &e) == 0 && a == 3 && b == 3);          // index.go:178-183
  CHECK(parse_part("2-5", 6, &a, &b, &e) == 1 && a == 2 && b == 5);        // :129-136
  CHECK(parse_part("5-2", 6, &a, &b, &e) == 1 && a == 5 && b == 2);        // end < start is not rejected
  CHECK(parse_part("2-3-x", 6, &a, &b, &e) == 1 && a == 2 && b == 3);      // Split: the third field is ignored
  CHECK(parse_part("+2-+3", 6, &a, &b, &e) == 1 && a == 2 && b == 3);
  CHECK(parse_part("0", 6, &a, &b, &e) == -1 && !strcmp(e, E_IDX_BOUNDS));
  CHECK(parse_part("7", 6, &a, &b, &e) == -1 && !strcmp(e, E_IDX_BOUNDS));
  CHECK(parse_part("", 6, &a, &b, &e) == -1 && !strcmp(e, E_IDX_BOUNDS));
  CHECK(parse_part("-2", 6, &a, &b, &e) == -1 && !strcmp(e, E_IDX_RANGE));  // ["", "2"]
  CHECK(parse_part("2-", 6, &a, &b, &e) == -1 && !strcmp(e, E_IDX_RANGE));
  CHECK(parse_part("1-7", 6, &a, &b, &e) == -1 && !strcmp(e, E_IDX_RANGE));
  CHECK(parse_part("5--3", 6, &a, &b, &e) == -1 && !strcmp(e, E_IDX_RANGE));  // ["5", "", "3"]
  CHECK(range_visits(0, 3, 3) == 1 && range_visits(1, 3, 3) == 1 && range_visits(1, 5, 2) == 0);
  CHECK(range_visits(1, 2, 5) == 4 && range_visits(1, 1, I64_MAX) == (u64)I64_MAX);
}

static void test_parse_parts() {
  const char *parts[] = {"2-4", "5-4", "3", "9", "x-1"};
  Parsed p = parse_parts(parts, 5, 6);
  CHECK(p.segs.size() == 3 && p.err_part == 3 && !strcmp(p.err, E_IDX_BOUNDS));  // nothing past the first error
  CHECK(p.visits == 4 && p.first_nonempty == 0);
  CHECK(p.segs[0].a0 == 1 && p.segs[0].b0 == 3 && p.segs[0].nr == 3 && p.segs[1].nr == 0 && p.segs[2].nr == 1);
  const char *empty[] = {"5-4", "3-1"};
  p = parse_parts(empty, 2, 6);
  CHECK(p.err_part == -1 && p.visits == 0 && p.first_nonempty == -1 && p.segs.size() == 2);
  p = parse_parts(nullptr, 0, 6);
  CHECK(p.err_part == -1 && p.segs.empty() && p.visits == 0);
  // visit counts saturate: 2^20 parts of 2^62 rows each do not wrap the sum
  std::vector<const char *> big(MAX_PARTS, "1-4611686018427387904");
  p = parse_parts(big.data(), big.size(), I64_MAX);
  CHECK(p.err_part == -1 && p.visits > MAX_VISITS);
}

static void test_size_part() {
  i64 pos = 0, len = 0;
  const char *e = nullptr;
  const i64 MiB = 1048576, size = 2 * MiB + MiB / 2;
  CHECK(size_part("1", size, MiB, &pos, &len, &e) == 0 && pos == 0 && len == MiB);            // virtual.go:72-77
  CHECK(size_part("3", size, MiB, &pos, &len, &e) == 0 && pos == 2 * MiB && len == MiB / 2);  // the last chunk
  CHECK(size_part("4", size, MiB, &pos, &len, &e) == -1 && !strcmp(e, E_IDX_BOUNDS));         // :68 one past it
  CHECK(size_part("1-3", size, MiB, &pos, &len, &e) == 0 && pos == 0 && len == size);         // :61-62 across the end
  CHECK(size_part("1-2", size, MiB, &pos, &len, &e) == 0 && pos == 0 && len == 2 * MiB);      // :63-64
  CHECK(size_part("1-4", size, MiB, &pos, &len, &e) == -1 && !strcmp(e, E_IDX_RANGE));
  CHECK(size_part("3-1", 20, 5, &pos, &len, &e) == 0 && pos == 10 && len == -5);  // end < start is not rejected
  CHECK(size_part("1", 0, 5, &pos, &len, &e) == 0 && pos == 0 && len == 0);
  CHECK(size_part("0", 9, 5, &pos, &len, &e) == -1 && size_part("x", 9, 5, &pos, &len, &e) == -1);
  CHECK(size_part("100", 100, 1, &pos, &len, &e) == 0 && pos == 99 && len == 1);
  CHECK(size_part("101", 100, 1, &pos, &len, &e) == 0 && pos == 100 && len == 0);
  CHECK(size_part("5", 100, 0, &pos, &len, &e) == 0 && pos == 0 && len == 0);      // chunk_size 0
  CHECK(size_part("2-9", 100, 0, &pos, &len, &e) == 0 && pos == 0 && len == 0);
  CHECK(size_part("3", 100, -1, &pos, &len, &e) == 0 && pos == -2 && len == -1);   // chunk_size -1
  const i64 big = 1ll << 62;  // products that wrap: 4 * 2^62 = 0, 2 * 2^62 = -2^63 (mod 2^64)
  CHECK(size_part("5", 10, big, &pos, &len, &e) == 0 && pos == 0 && len == 10);
  CHECK(size_part("3", 10, big, &pos, &len, &e) == 0 && pos == I64_MIN && len == I64_MIN + 10);
  CHECK(size_part("9223372036854775807", 9, 2, &pos, &len, &e) == 0 && pos == -4);  // (2^63-2)*2 = -4
  CHECK(size_part("2", 9, I64_MIN, &pos, &len, &e) == 0 && pos == I64_MIN);
}

static void test_chunk_segment() {
  u64 a0 = 9, nr = 9;
  CHECK(chunk_segment(0, 160, 40, &a0, &nr) && a0 == 0 && nr == 10);      // single.go:412-413: "1-10"
  CHECK(chunk_segment(160, 16, 40, &a0, &nr) && a0 == 10 && nr == 1);     // "11-11": one record
  CHECK(chunk_segment(175, 31, 40, &a0, &nr) && a0 == 10 && nr == 1);     // int64 division truncates
  CHECK(chunk_segment(320, 0, 40, &a0, &nr) && a0 == 20 && nr == 0);      // "21-20": empty
  CHECK(chunk_segment(320, 15, 40, &a0, &nr) && nr == 0);
  CHECK(!chunk_segment(0, 5, 40, &a0, &nr) && nr == 0);                   // "1-0": end <= 0
  CHECK(!chunk_segment(-32, 160, 40, &a0, &nr));                          // "-1-8": an empty first field
  CHECK(chunk_segment(-15, 160, 40, &a0, &nr) && a0 == 0 && nr == 10);    // -15/16 = 0 in Go
  CHECK(!chunk_segment(640, 16, 40, &a0, &nr));                           // start 41 > 40
  CHECK(!chunk_segment(560, 160, 40, &a0, &nr));                          // stop 45 > 40
  CHECK(chunk_segment(624, 16, 40, &a0, &nr) && a0 == 39 && nr == 1);     // the last record
  CHECK(!chunk_segment(16, -160, 40, &a0, &nr));                          // "2--9"
  // the quotients are below 2^59 in size, so (start-1) + c1/16 cannot wrap
  CHECK(chunk_segment(I64_MAX, I64_MAX, I64_MAX, &a0, &nr) && a0 == (1ull << 59) - 1 && nr == (1ull << 59) - 1);
  CHECK(!chunk_segment(I64_MIN, I64_MIN, I64_MAX, &a0, &nr));
  CHECK(chunk_segment(0, I64_MAX, I64_MAX, &a0, &nr) && a0 == 0 && nr == (u64)(I64_MAX / 16));
}

static void test_first_error() {
  const char *parts[] = {"1", "2-3", "9", "1"};
  const Parsed bad = parse_parts(parts, 4, 6);   // parse error at part 2
  const Parsed good = parse_parts(parts, 2, 6);
  PlanError e = first_error(good, ~0ull, -1);
  CHECK(e.part == -1 && e.text == nullptr);
  e = first_error(bad, ~0ull, -1);
  CHECK(e.part == 2 && !strcmp(e.text, E_IDX_BOUNDS));
  e = first_error(bad, (1ull << 32) | 5, -1);  // an invalid segment in part 1 comes first
  CHECK(e.part == 1 && !strcmp(e.text, E_IDX_RANGE));
  e = first_error(bad, 0, -1);                 // part 0, record 0
  CHECK(e.part == 0 && !strcmp(e.text, E_IDX_RANGE));
  e = first_error(good, (1ull << 32) | 7, -1);
  CHECK(e.part == 1 && !strcmp(e.text, E_IDX_RANGE));
  e = first_error(bad, ~0ull, bad.first_nonempty);  // the record index is missing: the first part that needs it
  CHECK(e.part == 0 && !strcmp(e.text, E_IDX_NOFILE));
  const char *late[] = {"3-2", "5-4", "2", "x"};
  const Parsed l = parse_parts(late, 4, 6);
  CHECK(l.first_nonempty == 2 && l.err_part == 3);
  e = first_error(l, ~0ull, l.first_nonempty);
  CHECK(e.part == 2 && !strcmp(e.text, E_IDX_NOFILE));
  const Parsed none = parse_parts(late, 2, 6);  // no part reaches level 2: a missing record index is no error
  e = first_error(none, ~0ull, none.first_nonempty);
  CHECK(e.part == -1);
}

int main() {
  test_parse_int();
  test_parse_part();
  test_parse_parts();
  test_size_part();
  test_chunk_segment();
  test_first_error();
  if (failures) {
    printf("plan_test: %d check(s) failed\n", failures);
    return 1;
  }
  printf("plan_test ok\n");
  return 0;
}
