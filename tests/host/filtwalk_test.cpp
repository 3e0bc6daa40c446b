// filtwalk_test.cpp -- CPU test of the download filters' slab walk arithmetic in
// shock_amd/csrc/sidx_filtwalk.hpp: the slab a device budget allows (at and just under the smallest
// budget, never over a budget), where a slab lies, the row cap against a slab of shortest records,
// the output bound at counters of 1, 8, 9 and 20 digits, the whole-path bounds and the restart /
// ENOMEM decision.
// Stand-alone: it includes that header only, links nothing of the library and makes no HIP call.
// Built with the host sanitizers by `make -C shock_amd/csrc filtwalk_test`; exit 0 = every check held.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "sidx_filtwalk.hpp"

using namespace sidx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

// a device model: a 144-byte carry rounded to 256, scan temporaries of 4 KiB, 32 KiB output blocks,
// a persistent grid of 2048 workgroups
static const FiltWalkDev DV = {256, 4096, 32768, 2048};

static void test_sizing() {
  CHECK(FILTWALK_MIN_BUDGET == (32ull << 20));
  const u64 size = 10ull << 30;
  const u64 h = filtwalk_default_halo(FILTWALK_MIN_BUDGET);
  CHECK(h > 0 && h % 4096 == 0 && h <= colwalk_default_halo(FILTWALK_MIN_BUDGET));
  CHECK(filtwalk_default_halo(1ull << 30) == COLWALK_HALO && filtwalk_default_halo(8ull << 30) == COLWALK_HALO);
  const u64 S = filtwalk_slab_bytes(FILTWALK_MIN_BUDGET, h, size, DV);
  CHECK(S >= FILTWALK_ALIGN && S % FILTWALK_ALIGN == 0);
  CHECK(S + h >= FILTWALK_DETECT);  // the first slab holds the bytes detection reads
  CHECK(filtwalk_slab_bytes(FILTWALK_MIN_BUDGET - 1, h, size, DV) == 0);
  CHECK(filtwalk_slab_bytes(0, h, size, DV) == 0);
  CHECK(filtwalk_slab_bytes(FILTWALK_MIN_BUDGET, 16ull << 20, size, DV) == 0);  // a halo that leaves no room
  // never over the budget, and the next slab size up would be
  for (u64 b = FILTWALK_MIN_BUDGET; b <= (64ull << 30); b += b / 3 + 12345) {
    const u64 halo = filtwalk_default_halo(b), s = filtwalk_slab_bytes(b, halo, size, DV);
    CHECK(s > 0 && s <= FILTWALK_MAX_SLAB);
    CHECK(filtwalk_footprint(s, halo, size, DV) <= b);
    if (s < FILTWALK_MAX_SLAB) CHECK(filtwalk_footprint(s + FILTWALK_ALIGN, halo, size, DV) > b);
    // the footprint covers every planned buffer
    const FiltWalkPlan p = filtwalk_plan(s, halo, size, DV);
    CHECK(2 * p.slot + p.view + 16 * p.rows + p.ws + p.out + DV.carry_bytes < filtwalk_footprint(s, halo, size, DV));
    CHECK(p.slot == s + halo + FILTWALK_PAD && p.view == s + halo + FILTWALK_PAD);
  }
  CHECK(filtwalk_slab_bytes(1ull << 42, COLWALK_HALO, size, DV) == FILTWALK_MAX_SLAB);
  // the whole path's bounds grow with the section and cover the section and its output
  CHECK(filtwalk_whole_bytes(96ull << 20, DV) > 2 * (96ull << 20));
  CHECK(filtwalk_whole_bytes(96ull << 20, DV) > FILTWALK_MIN_BUDGET);
  CHECK(filtwalk_whole_bytes(1ull << 30, DV) > filtwalk_whole_bytes(1ull << 29, DV));
  CHECK(filtwalk_whole_other_bytes(48ull << 20, DV) > FILTWALK_MIN_BUDGET);
  CHECK(filtwalk_whole_other_bytes(1ull << 20, DV) < (1ull << 30));
}

static void test_slab_positions() {
  const u64 S = 65536, H = 4096, n = 3 * 65536 + 100;
  FiltSlabPos p = filtwalk_slab_at(0, S, H, n, true);
  CHECK(p.lo == 0 && p.n == S && p.end == S + H && p.first && !p.last);
  p = filtwalk_slab_at(S, S, H, n, false);
  CHECK(p.lo == S && p.n == S && p.end == S + H && !p.first && !p.last);
  // the window reaches the section's end: the last slab, owning all of it
  p = filtwalk_slab_at(3 * S - 10, S, H, n, false);
  CHECK(p.last && p.lo + p.end == n && p.n == p.end && p.n == 110);
  p = filtwalk_slab_at(2 * S + 100, S, H, n, false);
  CHECK(p.last && p.end == S && p.n == S);
  p = filtwalk_slab_at(2 * S + 99 - H, S, H, n, false);
  CHECK(!p.last && p.n == S && p.end == S + H);  // one byte short of the end
  p = filtwalk_slab_at(0, S, H, 0, true);
  CHECK(p.last && p.n == 0 && p.end == 0);
  p = filtwalk_slab_at(n, S, H, n, false);
  CHECK(p.last && p.n == 0 && p.end == 0);
  CHECK(filtwalk_slot_bytes(S, H) == S + H + FILTWALK_PAD);
}

// the shortest records GetReadOffset accepts, back to back: the row cap holds them all
static void test_row_cap() {
  CHECK(FILTWALK_MIN_RECORD == 9);
  const std::string rec = "@a\nA\n+\nI\n";
  CHECK(rec.size() == FILTWALK_MIN_RECORD);
  for (u64 k : {0ull, 1ull, 2ull, 7ull, 1000ull, 116509ull}) {
    // k whole records, and the same with the last one's final '\n' missing (the section's end)
    CHECK(filtwalk_rows_cap(k * rec.size()) >= k);
    if (k) CHECK(filtwalk_rows_cap(k * rec.size() - 1) >= k);
    CHECK(filtwalk_rows_cap(k * rec.size()) <= k + 1);
  }
  CHECK(filtwalk_rows_cap((1ull << 20) + 4096) == ((1ull << 20) + 4096) / 9 + 1);
  CHECK(filtwalk_max_counter(9 * 1000) >= 1000);
}

// anonymize of the shortest record with counter c: "@" c "\n" "A" "\n+\n" "I" "\n"
static void test_out_bound() {
  CHECK(filtwalk_ndigits(0) == 1 && filtwalk_ndigits(9) == 1 && filtwalk_ndigits(10) == 2);
  CHECK(filtwalk_ndigits(99999999ull) == 8 && filtwalk_ndigits(100000000ull) == 9);
  CHECK(filtwalk_ndigits(~0ull) == 20 && filtwalk_ndigits(9999999999999999999ull) == 19);
  const u64 ctrs[] = {1, 9, 99999999ull, 100000000ull, 999999999ull, 10000000000000000000ull, ~0ull};
  for (u64 cmax : ctrs) {
    const u32 nd = filtwalk_ndigits(cmax);
    for (u64 k : {1ull, 3ull, 1000ull}) {
      const u64 in = 9 * k, out_anon = k * (8 + nd), out_fq2fa = k * 5;  // (every counter as long as the largest)
      const u64 bound = filtwalk_out_bound(in, k, cmax);
      CHECK(bound >= out_anon && bound >= out_fq2fa);
      CHECK(bound == in + (u64)(nd - 1) * k);
    }
  }
  CHECK(filtwalk_out_bound(900, 100, 1) == 900);                    // 1 digit: no longer than the input
  CHECK(filtwalk_out_bound(900, 100, 99999999ull) == 900 + 700);    // 8 digits
  CHECK(filtwalk_out_bound(900, 100, 100000000ull) == 900 + 800);   // 9 digits
  CHECK(filtwalk_out_bound(900, 100, ~0ull) == 900 + 1900);         // 20 digits
  // a record with a longer ID only shortens: "@abc\nA\n+abc\nI\n" (15 bytes) -> "@7\nA\n+\nI\n" (9)
  CHECK(filtwalk_out_bound(15, 1, 7) >= 9);
  // the workspace holds the spans, lengths, offsets, scan space and the output blocks' first records
  CHECK(filtwalk_ws_bytes(1000, 17000, 4096, 32768) >= 24 * 1001 + 16 * 1001 + 4096 + 8 * 4);
  CHECK(filtwalk_ws_bytes(0, 0, 0, 32768) % 256 == 0);
}

static void test_next() {
  // the slab at 1000 was followed by one staged from 5000
  CHECK(filtwalk_next(1000, 5000, 5000) == FiltNext::Continue);
  CHECK(filtwalk_next(1000, 5000, 5300) == FiltNext::Continue);  // the straddling record closed inside the halo
  CHECK(filtwalk_next(1000, 5000, 4999) == FiltNext::Restart);   // an owned record the halo did not settle
  CHECK(filtwalk_next(1000, 5000, 1001) == FiltNext::Restart);
  CHECK(filtwalk_next(1000, 5000, 1000) == FiltNext::NoMem);     // it already heads the slot
  CHECK(filtwalk_next(0, 65536, 0) == FiltNext::NoMem);
  // a restarted slab that makes progress goes on; one that does not ends the walk
  CHECK(filtwalk_next(4999, 4999 + 65536, 4999 + 70000) == FiltNext::Continue);
  CHECK(filtwalk_next(4999, 4999 + 65536, 4999) == FiltNext::NoMem);
}

int main() {
  test_sizing();
  test_slab_positions();
  test_row_cap();
  test_out_bound();
  test_next();
  if (failures) {
    printf("filtwalk_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("filtwalk_test ok\n");
  return 0;
}
