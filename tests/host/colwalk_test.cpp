// colwalk_test.cpp -- CPU test of the column slab walk's arithmetic in
// shock_amd/csrc/sidx_colwalk.hpp: the slab a device budget allows (at and just under the smallest
// budget, never over the budget; the shared bisect on its own), where a slab lies in its slot, the one retry rule (shorten /
// advance / no slot can hold the line) and the row cursor.
// Stand-alone: it includes that header only, links nothing of the library and makes no HIP call.
// Built with the host sanitizers by `make -C shock_amd/csrc colwalk_test`; exit 0 = every check held.
#include <stdint.h>
#include <stdio.h>

#include "sidx_colwalk.hpp"

using namespace sidx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

// a workspace model shaped like sidx_col_tile_bytes: a u16 per two input bytes, 44 bytes of words
// per tile, scan space, rounding
static u64 ws_model(u64 nt) { return 4096 + nt * (TILE + 44) + 8 * ((nt + 255) / 256) * 256; }
static const u64 CARRY = 64 + 2 * (32 + COL_KEYCAP);

static void test_sizing() {
  // the smallest budget the sizing accepts is 32 MiB: a 64 MiB node then needs the walk
  CHECK(COLWALK_MIN_BUDGET <= (32ull << 20));
  const u64 h = colwalk_default_halo(COLWALK_MIN_BUDGET);
  CHECK(h == (2ull << 20) && colwalk_default_halo(1ull << 30) == COLWALK_HALO && colwalk_default_halo(64ull << 20) == COLWALK_HALO);
  const u64 S = colwalk_slab_bytes(COLWALK_MIN_BUDGET, h, CARRY, ws_model);
  CHECK(S >= COLWALK_ALIGN && S % COLWALK_ALIGN == 0 && S % TILE == 0);
  CHECK(colwalk_slab_bytes(COLWALK_MIN_BUDGET - 1, h, CARRY, ws_model) == 0);
  CHECK(colwalk_slab_bytes(0, h, CARRY, ws_model) == 0);
  // a halo that leaves no room for a slab
  CHECK(colwalk_slab_bytes(COLWALK_MIN_BUDGET, 16ull << 20, CARRY, ws_model) == 0);
  // never over the budget, and the next slab size up would be
  for (u64 b = COLWALK_MIN_BUDGET; b <= (16ull << 30); b += b / 3 + 12345) {
    const u64 halo = colwalk_default_halo(b), s = colwalk_slab_bytes(b, halo, CARRY, ws_model);
    CHECK(s > 0 && s <= (1ull << 30));
    CHECK(colwalk_footprint(s, halo, CARRY, ws_model) <= b);
    CHECK(2 * colwalk_slot_bytes(s, halo) <= b);
    if (s < (1ull << 30)) CHECK(colwalk_footprint(s + COLWALK_ALIGN, halo, CARRY, ws_model) > b);
  }
  CHECK(colwalk_slab_bytes(1ull << 40, COLWALK_HALO, CARRY, ws_model) == (1ull << 30));
  CHECK(colwalk_rows_cap(0) == 4096 && colwalk_rows_cap(1ull << 20) == 32768 + 4096);
  CHECK(colwalk_slot_bytes(TILE, 4096) == COLWALK_FRONT + TILE + 4096 + COLWALK_PAD);
}

// the bisect the three walks' sizing shares (largest_slab, sidx_slabwalk.hpp)
static void test_largest_slab() {
  u64 calls = 0;
  CHECK(largest_slab(4096, 1ull << 30, [&](u64) { ++calls; return false; }) == 0 && calls > 0);  // fits nothing
  CHECK(largest_slab(4096, 1ull << 30, [](u64) { return true; }) == (1ull << 30));               // fits everything
  CHECK(largest_slab(1000, 4500, [](u64) { return true; }) == 4000);  // a max off a multiple: the multiple below it
  // a threshold S <= T: the largest multiple of align that is <= min(T, max), T on and off a multiple
  const u64 aligns[] = {1, 4096, 1ull << 20}, maxes[] = {1ull << 20, 256ull << 20, 1ull << 30};
  for (u64 align : aligns)
    for (u64 max : maxes) {
      const u64 qs[] = {0, 1, 2, 77, max / align - 1, max / align, max / align + 1, 4 * (max / align)};
      const u64 offs[] = {0, 1, align / 2, align - 1};
      for (u64 q : qs)
        for (u64 off : offs) {
          if (off >= align) continue;  // (align 1 has only T on a multiple)
          const u64 T = q * align + off, top = T < max ? T : max;
          u64 asked_over = 0;
          const u64 S = largest_slab(align, max, [&](u64 s) { asked_over += s > max || s % align != 0 || s == 0; return s <= T; });
          CHECK(S == top / align * align);
          CHECK(asked_over == 0);  // the predicate only ever sees positive multiples within max
        }
    }
}

static void test_slabs() {
  const u64 size = 200000, S = 3 * TILE, halo = 4096;
  ColSlabPos p = colwalk_slab_at(0, S, halo, size);
  CHECK(p.lo == 0 && p.n == S && p.end == S + halo && p.front == 0 && p.first && !p.last);
  p = colwalk_slab_at(S, S, halo, size);
  CHECK(p.n == S && p.end == S + halo && p.front == COLWALK_FRONT && !p.first && !p.last);
  p = colwalk_slab_at(4 * S, S, halo, size);  // the file ends inside it
  CHECK(p.n == size - 4 * S && p.end == p.n && p.last && !p.first);
  p = colwalk_slab_at(size - S - 100, S, halo, size);  // the halo is cut at the file's end
  CHECK(p.n == S && p.end == S + 100 && !p.last);
  p = colwalk_slab_at(5, S, halo, size);  // inside the file's first 16 bytes: nothing is read before it
  CHECK(p.front == 0 && !p.first);
  p = colwalk_slab_at(size - 1, S, halo, size);
  CHECK(p.n == 1 && p.end == 1 && p.last);
  // a halo of "the rest of the file"
  p = colwalk_slab_at(S, S, size, size);
  CHECK(p.end == size - S && !p.last);
  // shortened: the same window start, fewer owned bytes, no longer the last
  const ColSlabPos q = colwalk_slab_at(4 * S, S, halo, size);
  const ColSlabPos r = colwalk_shorten(q, 100, halo, size);
  CHECK(r.lo == q.lo && r.front == q.front && r.n == 100 && r.end == size - q.lo && !r.last && q.last);
  const ColSlabPos r2 = colwalk_shorten(colwalk_slab_at(S, S, halo, size), 100, halo, size);
  CHECK(r2.n == 100 && r2.end == 100 + halo && r2.front == COLWALK_FRONT);
}

static void test_retry() {
  u64 cut = 77;
  // the line at x follows the '\n' at x - 1: the slab keeps [lo, x - 1), the next starts at x - 1
  CHECK(colwalk_on_more(1000, 5000, &cut) == ColRetry::Shorten && cut == 4999);
  CHECK(colwalk_on_more(1000, 1002, &cut) == ColRetry::Shorten && cut == 1001);  // a one-byte slab is left
  CHECK(colwalk_on_more(0, 2, &cut) == ColRetry::Shorten && cut == 1);
  cut = 77;
  // x - 1 == lo: the line heads the slot and still does not fit
  CHECK(colwalk_on_more(1000, 1001, &cut) == ColRetry::NoMem && cut == 77);
  // the line at offset 0 has no '\n' before it
  CHECK(colwalk_on_more(0, 0, &cut) == ColRetry::NoMem);
  CHECK(colwalk_on_more(0, 1, &cut) == ColRetry::NoMem && cut == 77);
  CHECK(colwalk_on_more(UINT64_MAX - 1, UINT64_MAX, &cut) == ColRetry::NoMem);
  // the walk advances: a shortened slab owns at least one byte, and the next slab starts past lo
  for (u64 lo = 0; lo < 40; ++lo)
    for (u64 x = 0; x < 60; ++x)
      if (colwalk_on_more(lo, x, &cut) == ColRetry::Shorten) CHECK(cut > lo && cut == x - 1);
  // rows grown on ESPACE hold what the slab needs, and always grow
  CHECK(colwalk_grow_rows(100, 101) >= 101 && colwalk_grow_rows(4096, 1000000) >= 1000000);
  CHECK(colwalk_grow_rows(5000, 10) > 5000);
}

static void test_cursor() {
  ColRowCursor cur;
  CHECK(cur.total == 0 && cur.file_pos() == 0);
  CHECK(cur.take(0) == 0 && cur.file_pos() == 0);  // a slab without a cut
  CHECK(cur.take(5) == 0 && cur.total == 5 && cur.file_pos() == 80);
  CHECK(cur.take(1) == 5 && cur.file_pos() == 96);
  CHECK(cur.take(1ull << 32) == 6 && cur.file_pos() == 16 * ((1ull << 32) + 6));  // past 2^32 rows, past 2^36 bytes
}

int main() {
  test_sizing();
  test_largest_slab();
  test_slabs();
  test_retry();
  test_cursor();
  if (failures) {
    printf("colwalk_test: %d checks failed\n", failures);
    return 1;
  }
  printf("colwalk_test ok\n");
  return 0;
}
