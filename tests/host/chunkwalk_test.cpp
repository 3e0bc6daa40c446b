// chunkwalk_test.cpp -- CPU test of the chunkrecord slab walk's arithmetic in
// shock_amd/csrc/sidx_chunkwalk.hpp: where slot k lies, the slab a device budget allows (at and just
// under the smallest budget, never over the budget), the per-slab row bound, and the carry's
// precondition -- with the proof obligation that H >= WIN satisfies it for consecutive slots, checked
// by walking a model of the serial walk (any window either matches or not) through the slots.
// Stand-alone: it includes that header only, links nothing of the library and makes no HIP call.
// Built with the host sanitizers by `make -C shock_amd/csrc chunkwalk_test`; exit 0 = every check held.
#include <stdint.h>
#include <stdio.h>

#include "sidx_chunkwalk.hpp"

using namespace sidx;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static const ChunkWalkDev DEV = {256, 4096, 64, 1024};

static void test_slots() {
  const u64 H = CHUNKWALK_HALO;
  // every byte lies in some slot's owned part, slots go in file order, each reads H before its slab
  for (u64 n : {0ull, 1ull, 65535ull, 65536ull, 65537ull, 1000000ull, (3ull << 20) + 5, 6ull << 20}) {
    for (u64 S : {65536ull, 262144ull, 1ull << 20, 99984ull}) {
      const u64 K = chunkwalk_slots(S, n);
      CHECK(K >= 1 && (n == 0 ? K == 1 : (K - 1) * S < n && K * S >= n));
      u64 prev_hi = 0;
      for (u64 k = 0; k < K; ++k) {
        const ChunkSlot p = chunkwalk_slot(k, S, n);
        CHECK(p.base == k * S && p.lo == (k * S < H ? 0 : k * S - H) && p.hi == (n - k * S < S ? n : (k + 1) * S));
        CHECK(p.front == p.base - p.lo && p.end == p.hi - p.base && p.lo + p.front + p.end == p.hi);
        CHECK(p.first == (p.lo == 0) && p.last == (p.hi == n) && p.last == (k + 1 == K));
        CHECK(p.hi - p.lo + CHUNKWALK_PAD <= chunkwalk_slot_bytes(S));
        if (k) CHECK(p.base == prev_hi && p.lo + CHUNKWALK_WIN <= prev_hi);  // the next slot reaches back past the window
        prev_hi = p.hi;
      }
      CHECK(prev_hi == n);
    }
  }
  CHECK(chunkwalk_slot(0, 1 << 20, 10).last && chunkwalk_slot(0, 1 << 20, 10).hi == 10);
}

// The serial walk over the slots with windows that match (bit set in the pattern) or do not: the
// carry that leaves slot k always enters slot k + 1, no window is evaluated twice or skipped, and a
// slab emits at most its row bound -- for chunks from the smallest to larger than a slab, and for
// stretches without a match longer than several slots.
static void test_carry_and_bound() {
  const u64 WIN = CHUNKWALK_WIN;
  for (u64 chunk : {WIN, WIN + 1, 40000ull, 65536ull, 1ull << 20, (1ull << 20) + 77}) {
    for (u64 S : {65536ull, 131072ull, 262144ull}) {
      for (u64 pattern : {0x0ull, ~0ull, 0x5555555555555555ull, 0x0000ffff0000ffffull, 0x1ull}) {
        const u64 n = 5 * S + 12345;
        u64 curr = 0, off = 0, evaluated = 0, rows = 0, win_i = 0;
        bool done = false;
        const u64 K = chunkwalk_slots(S, n);
        for (u64 k = 0; k < K; ++k) {
          const ChunkSlot p = chunkwalk_slot(k, S, n);
          CHECK(!done && chunkwalk_carry_enters(off, chunk, p.lo));
          const u64 from = curr > p.lo ? curr : p.lo;
          u64 emitted = 0;
          for (;;) {
            const u64 w = off + chunk - WIN;
            if (w + WIN > p.hi) {
              if (p.last) { ++emitted; done = true; }
              break;
            }
            CHECK(w >= p.lo);
            ++evaluated;
            if ((pattern >> (win_i++ & 63)) & 1) {  // a match: the shortest chunk the rule allows (pos = 1)
              curr = w + 1;
              off = curr;
              ++emitted;
            } else {
              off += WIN;
            }
          }
          CHECK(emitted <= chunkwalk_row_bound(p.hi - from, chunk));
          CHECK(emitted <= chunkwalk_row_bound(p.hi - p.lo, chunk));
          rows += emitted;
        }
        CHECK(done && rows >= 1 && evaluated == win_i);
      }
    }
  }
  CHECK(!chunkwalk_carry_enters(0, CHUNKWALK_WIN, 1) && chunkwalk_carry_enters(1, CHUNKWALK_WIN, 1));
  CHECK(chunkwalk_carry_enters(0, 1 << 20, (1 << 20) - CHUNKWALK_WIN) && !chunkwalk_carry_enters(0, 1 << 20, (1 << 20) - CHUNKWALK_WIN + 1));
  CHECK(chunkwalk_row_bound(0, CHUNKWALK_WIN) == 2 && chunkwalk_row_bound(10, CHUNKWALK_WIN) == 12);
  CHECK(chunkwalk_row_bound(1 << 20, 1 << 20) == 3);
}

static void test_sizing() {
  const u64 chunk = 1 << 20;
  CHECK(CHUNKWALK_MIN_BUDGET == (32ull << 20));
  const u64 S = chunkwalk_slab_bytes(CHUNKWALK_MIN_BUDGET, chunk, DEV);
  CHECK(S >= CHUNKWALK_ALIGN && S % CHUNKWALK_ALIGN == 0);
  CHECK(chunkwalk_slab_bytes(CHUNKWALK_MIN_BUDGET - 1, chunk, DEV) == 0);
  CHECK(chunkwalk_slab_bytes(0, chunk, DEV) == 0);
  // never over the budget, and the next slab size up would be; a small chunk's rows take their share
  for (u64 ch : {CHUNKWALK_WIN + 1, 65536ull, chunk}) {
    for (u64 b = CHUNKWALK_MIN_BUDGET; b <= (16ull << 30); b += b / 3 + 12345) {
      const u64 s = chunkwalk_slab_bytes(b, ch, DEV);
      if (!s) {  // (the rows of a tiny chunk leave no room under a small budget)
        CHECK(chunkwalk_footprint(CHUNKWALK_ALIGN, ch, DEV) > b);
        continue;
      }
      CHECK(s <= CHUNKWALK_MAX_SLAB && chunkwalk_footprint(s, ch, DEV) <= b && 2 * chunkwalk_slot_bytes(s) <= b);
      if (s < CHUNKWALK_MAX_SLAB) CHECK(chunkwalk_footprint(s + CHUNKWALK_ALIGN, ch, DEV) > b);
    }
  }
  CHECK(chunkwalk_slab_bytes(1ull << 40, chunk, DEV) == CHUNKWALK_MAX_SLAB);
  // the footprint grows with the slab, and its parts with the view
  for (u64 s = CHUNKWALK_ALIGN; s < (64ull << 20); s += 7 * CHUNKWALK_ALIGN) {
    CHECK(chunkwalk_footprint(s, chunk, DEV) < chunkwalk_footprint(s + CHUNKWALK_ALIGN, chunk, DEV));
    CHECK(chunkwalk_cra_bytes(s, DEV.scan_bytes, DEV.gslot) <= chunkwalk_cra_bytes(s + 1, DEV.scan_bytes, DEV.gslot));
    CHECK(chunkwalk_crb_bytes(s, chunk) <= chunkwalk_crb_bytes(s + 1, chunk));
  }
  // the whole-node build of a node holds more than the node, and more than a walk's footprint
  CHECK(chunkwalk_whole_bytes(96ull << 20, chunk, DEV) > (96ull << 20));
  CHECK(chunkwalk_whole_bytes(96ull << 20, chunk, DEV) > (32ull << 20));
  CHECK(chunkwalk_whole_bytes(10ull << 30, chunk, DEV) > (11ull << 30));
  CHECK(chunkwalk_nodes_cap(0) == 4096 && chunkwalk_nodes_cap(1 << 20) == 8192 + 4096);
}

int main() {
  test_slots();
  test_carry_and_bound();
  test_sizing();
  if (failures) {
    printf("chunkwalk_test: %d check(s) failed\n", failures);
    return 1;
  }
  printf("chunkwalk_test ok\n");
  return 0;
}
