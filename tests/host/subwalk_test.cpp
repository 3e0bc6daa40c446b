// subwalk_test.cpp -- CPU test of the subset walk's arithmetic in shock_amd/csrc/sidx_subwalk.hpp:
// the id slab and the parent window a device budget allows (at and just under the smallest budget,
// never over the budget), the window that follows a stop at an id, the rule for a line that does
// not close (restart from it / no slot can hold it) and the row and run cursors.
// Stand-alone: it includes that header only, links nothing of the library and makes no HIP call.
// Built with the host sanitizers by `make -C shock_amd/csrc subwalk_test`; exit 0 = every check held.
#include <stdint.h>
#include <stdio.h>

#include "sidx_subwalk.hpp"

using namespace sidx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

// a workspace model shaped like subset_slab_ws_bytes: 8 bytes per text byte for the line ends, 12
// per KiB block, seven 8-byte arrays for a line per byte at worst, scan space, rounding
static u64 ws_model(u64 end) { return 8 * (end + 2) + 12 * ((end + 1023) / 1024) + 56 * (end + 1) + end / 128 + 8192; }
static const u64 CARRY = 256;

static void test_sizing() {
  CHECK(SUBWALK_MIN_BUDGET == (32ull << 20) && SUBWALK_HALO == 65536);
  const u64 pc = 500000;
  const u64 W = subwalk_window_rows(SUBWALK_MIN_BUDGET, pc);
  CHECK(W == pc);  // 8 MB: the whole index fits a quarter of 32 MiB
  CHECK(subwalk_window_rows(SUBWALK_MIN_BUDGET, 10000000) == (SUBWALK_MIN_BUDGET / 64));
  CHECK(subwalk_window_rows(SUBWALK_MIN_BUDGET, 0) == 1);
  const u64 S = subwalk_slab_bytes(SUBWALK_MIN_BUDGET, SUBWALK_HALO, W, CARRY, ws_model);
  CHECK(S >= SUBWALK_ALIGN && S % SUBWALK_ALIGN == 0);
  CHECK(subwalk_slab_bytes(SUBWALK_MIN_BUDGET - 1, SUBWALK_HALO, W, CARRY, ws_model) == 0);
  CHECK(subwalk_slab_bytes(0, SUBWALK_HALO, W, CARRY, ws_model) == 0);
  // a window that leaves no room for a slab
  CHECK(subwalk_slab_bytes(SUBWALK_MIN_BUDGET, SUBWALK_HALO, SUBWALK_MIN_BUDGET / 16, CARRY, ws_model) == 0);
  // never over the budget, and the next slab size up would be (unless the largest slab is reached)
  for (u64 b = SUBWALK_MIN_BUDGET; b <= (64ull << 30); b += b / 3 + 12345) {
    for (u64 rows : {0ull, 1000ull, 78000000ull, 1ull << 33}) {
      const u64 w = subwalk_window_rows(b, rows);
      CHECK(16 * w <= b / 4 || w == 1);
      const u64 s = subwalk_slab_bytes(b, SUBWALK_HALO, w, CARRY, ws_model);
      CHECK(s > 0 && s <= SUBWALK_MAX_SLAB);
      CHECK(subwalk_footprint(s, SUBWALK_HALO, w, CARRY, ws_model) <= b);
      if (s < SUBWALK_MAX_SLAB) CHECK(subwalk_footprint(s + SUBWALK_ALIGN, SUBWALK_HALO, w, CARRY, ws_model) > b);
    }
  }
  // the tables are never short: a slab of S bytes holds at most S / 2 + 1 lines of two bytes or more
  for (u64 s : {1ull, 2ull, 3ull, 64ull, 65537ull}) {
    CHECK(subwalk_rows_cap(s) >= s / 2 + 1 && subwalk_runs_cap(s) >= subwalk_rows_cap(s) + 1);
  }
  // the C4 case of the issue: 700 MB of ids over 156 M parent rows under 8 GiB
  const u64 w4 = subwalk_window_rows(8ull << 30, 156000000);
  const u64 s4 = subwalk_slab_bytes(8ull << 30, SUBWALK_HALO, w4, CARRY, ws_model);
  CHECK(w4 == (8ull << 30) / 64 && s4 >= (32ull << 20));
  CHECK(subwalk_footprint(s4, SUBWALK_HALO, w4, CARRY, ws_model) <= (8ull << 30));
}

static void test_windows() {
  // the first window starts at row 0
  SubWindow w = subwalk_window_at(0, 4096, 10000);
  CHECK(w.row0 == 0 && w.rows == 4096);
  // after a stop at id 4097 (dense): the windows abut
  w = subwalk_next_window(4097, 4096, 10000);
  CHECK(w.row0 == 4096 && w.rows == 4096);
  // a sparse list skips rows; the last window is short
  w = subwalk_next_window(9000, 4096, 10000);
  CHECK(w.row0 == 8999 && w.rows == 1001);
  w = subwalk_next_window(10000, 4096, 10000);
  CHECK(w.row0 == 9999 && w.rows == 1);
  w = subwalk_next_window(1, 1, 10000);
  CHECK(w.row0 == 0 && w.rows == 1);
  // never past the table
  w = subwalk_window_at(20000, 4096, 10000);
  CHECK(w.row0 == 10000 && w.rows == 0);
  w = subwalk_window_at(0, 4096, 0);
  CHECK(w.row0 == 0 && w.rows == 0);
  // past 2^32 rows
  w = subwalk_next_window((int64_t)((1ull << 33) + 5), 1ull << 20, 1ull << 34);
  CHECK(w.row0 == (1ull << 33) + 4 && w.rows == (1ull << 20));
}

static void test_open_line() {
  // a line inside the slab that does not close: the next slab starts at it
  CHECK(subwalk_on_open_line(1000, 1500) == SubRetry::Restart);
  CHECK(subwalk_on_open_line(0, 4) == SubRetry::Restart);
  // the line heads the slot (or the file) and still does not close: no slot can hold it
  CHECK(subwalk_on_open_line(1000, 1000) == SubRetry::NoMem);
  CHECK(subwalk_on_open_line(0, 0) == SubRetry::NoMem);
  // the slab that restarts at an open line sits in its slot like any other
  const ColSlabPos p = colwalk_slab_at(1500, 65536, SUBWALK_HALO, 1000000);
  CHECK(p.lo == 1500 && p.n == 65536 && p.end == 65536 + SUBWALK_HALO && p.front == COLWALK_FRONT && !p.first && !p.last);
  const ColSlabPos q = colwalk_slab_at(4, 65536, SUBWALK_HALO, 100);
  CHECK(q.n == 96 && q.end == 96 && q.front == 0 && q.last && !q.first);
}

static void test_cursors() {
  SubCursor cur;
  CHECK(cur.rows == 0 && cur.runs == 0 && cur.rows_pos() == 0 && cur.runs_pos() == 0);
  CHECK(cur.take_rows(0) == 0 && cur.take_runs(0) == 0);  // a call that only closes nothing
  CHECK(cur.take_rows(5) == 0 && cur.rows == 5 && cur.rows_pos() == 80 && cur.runs_pos() == 0);
  CHECK(cur.take_runs(2) == 0 && cur.take_runs(1) == 2 && cur.runs_pos() == 48);
  CHECK(cur.take_rows(1ull << 32) == 5 && cur.rows_pos() == 16 * ((1ull << 32) + 5));  // past 2^32 rows, past 2^36 bytes
}

int main() {
  test_sizing();
  test_windows();
  test_open_line();
  test_cursors();
  if (failures) {
    printf("subwalk_test: %d checks failed\n", failures);
    return 1;
  }
  printf("subwalk_test ok\n");
  return 0;
}
