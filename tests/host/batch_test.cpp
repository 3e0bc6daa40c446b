// batch_test.cpp -- CPU test of the batch build's host arithmetic in
// shock_amd/csrc/sidx_batch_host.hpp: which {pos, len} a batch accepts (alignment, range, overflow of
// pos + len), the packing of node bodies into one arena, the small-node limit, a single node's row
// region and the split of a list into batched nodes and singles.
// Stand-alone: it includes that header only, links nothing of the library and makes no HIP call.
// Built with the host sanitizers by `make -C shock_amd/csrc batch_test` (an unsigned wrap that
// mattered would show as a wrong value, a signed one as a UBSan report); exit 0 = every check held.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "sidx_batch_host.hpp"

using namespace sidx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static void test_node_ok() {
  const uint64_t n = 4096;
  CHECK(batch_node_ok(0, 0, n) && batch_node_ok(0, 4096, n) && batch_node_ok(4096, 0, n));
  CHECK(batch_node_ok(16, 4080, n) && !batch_node_ok(16, 4081, n));
  CHECK(!batch_node_ok(-16, 1, n) && !batch_node_ok(16, -1, n));
  CHECK(!batch_node_ok(8, 1, n) && !batch_node_ok(1, 0, n) && !batch_node_ok(4095, 0, n));  // misaligned
  CHECK(!batch_node_ok(4112, 0, n));                                                          // pos past the end
  CHECK(!batch_node_ok(16, INT64_MAX, n) && !batch_node_ok(INT64_MAX - 15, 16, n));          // pos + len wraps
  CHECK(batch_node_ok(0, 0, 0) && !batch_node_ok(0, 1, 0) && !batch_node_ok(16, 0, 0));
  CHECK(batch_node_ok(INT64_MAX - 15, 15, UINT64_MAX));
}

static void test_small() {
  CHECK(batch_is_small(0, 4096) && batch_is_small(4096, 4096) && !batch_is_small(4097, 4096));
  CHECK(!batch_is_small(0, 0) && !batch_is_small(1, 0));  // limit 0: every node is a single
  CHECK(batch_small_limit(nullptr, 77) == 77 && batch_small_limit("", 77) == 77 && batch_small_limit("x", 77) == 77);
  CHECK(batch_small_limit("0", 77) == 0 && batch_small_limit("4096", 77) == 4096 && batch_small_limit("12k", 77) == 12);
}

static void test_pack() {
  const uint64_t lens[] = {0, 1, 15, 16, 17, 0, 1000};
  uint64_t pos[7], arena = 1;
  CHECK(batch_pack(lens, 7, pos, &arena));
  const uint64_t want[] = {0, 0, 16, 32, 48, 80, 80};
  for (int i = 0; i < 7; ++i) CHECK(pos[i] == want[i] && pos[i] % 16 == 0);
  CHECK(arena == 80 + 1008 && arena % 16 == 0);
  for (int i = 0; i < 7; ++i) CHECK(batch_node_ok((int64_t)pos[i], (int64_t)lens[i], arena));
  for (int i = 0; i + 1 < 7; ++i) CHECK(pos[i] + lens[i] <= pos[i + 1]);  // no overlap
  CHECK(batch_pack(lens, 0, pos, &arena) && arena == 0);
  const uint64_t huge[] = {1ull << 62, 1ull << 62};
  CHECK(!batch_pack(huge, 2, pos, &arena));  // the arena would not fit an int64 position
  const uint64_t wrap[] = {16, UINT64_MAX - 8};
  CHECK(!batch_pack(wrap, 2, pos, &arena));
  const uint64_t edge[] = {(1ull << 63) - 32};
  CHECK(batch_pack(edge, 1, pos, &arena) && arena == (1ull << 63) - 32);
}

static void test_rows() {
  CHECK(batch_region_rows(0, 10, 10) == 10 && batch_region_rows(4, 4, 10) == 0 && batch_region_rows(4, 9, 10) == 5);
  CHECK(batch_region_rows(9, 4, 10) == 0 && batch_region_rows(4, 11, 10) == 0);  // an inconsistent layout: nothing
  uint64_t r = 0;
  CHECK(batch_rows_guess(0, 0, &r) && r == 64);
  CHECK(batch_rows_guess(1600, 10, &r) && r == 100 + 20 + 64);
  CHECK(!batch_rows_guess(0, (1ull << 58) + 1, &r) && !batch_rows_guess(UINT64_MAX, 0, &r));
  CHECK(batch_rows_guess(1ull << 62, 1ull << 40, &r) && r < (1ull << 59));
}

static void test_split() {
  BatchSplit s;
  CHECK(batch_split(10, 0, &s) && s.batches == 1 && s.batched == 10 && s.singles == 0);
  CHECK(batch_split(10, 3, &s) && s.batches == 1 && s.batched == 7 && s.singles == 3);
  CHECK(batch_split(10, 10, &s) && s.batches == 0 && s.batched == 0 && s.singles == 10);
  CHECK(batch_split(0, 0, &s) && s.batches == 0);
  CHECK(!batch_split(3, 4, &s));
}

int main() {
  test_node_ok();
  test_small();
  test_pack();
  test_rows();
  test_split();
  if (failures) {
    printf("batch_test: %d check(s) failed\n", failures);
    return 1;
  }
  printf("batch_test ok\n");
  return 0;
}
