// claim_test.cpp -- CPU test of the tile passes' claim plan (shock_amd/csrc/sidx_claim.hpp): for
// every tile count and grid below, the claims are non-empty, in file order and partition the tiles
// exactly; every claim starts at an even tile and holds at most 32; the claim after the last is
// empty; the batch size follows its rule.  Stand-alone: it includes that header only, links
// nothing of the library and makes no HIP call.  Built with the host sanitizers by
// `make -C shock_amd/csrc claim_test`; exit 0 = every check held.
#include <stdio.h>

#include "sidx_claim.hpp"

using namespace sidx;

static int failures = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (failures < 20) printf("%s:%d: CHECK failed: %s (ntiles %u G %u)\n", __FILE__, __LINE__, #cond, nt_, G_); \
      ++failures;                                                                          \
    }                                                                                      \
  } while (0)

static uint32_t nt_, G_;

static uint64_t cdiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// the rule, written out: the largest of 32, 16, 8, 4, 2 with ceil(ntiles / B) >= 4 G, else 2
static uint32_t expect_B(uint32_t ntiles, uint32_t G) {
  for (uint32_t B : {32u, 16u, 8u, 4u, 2u})
    if (cdiv(ntiles, B) >= 4ull * G) return B;
  return 2;
}

static void check(uint32_t ntiles, uint32_t G) {
  nt_ = ntiles;
  G_ = G;
  const ClaimPlan pl = claim_plan(ntiles, G);
  CHECK(pl.B == expect_B(ntiles, G));
  const uint64_t nb = cdiv(ntiles, pl.B);
  CHECK(pl.nmain == (nb > G ? nb - G : 0));
  const uint32_t tb_want = pl.B / CLAIM_TAIL_DIV > 2 ? pl.B / CLAIM_TAIL_DIV : 2;
  CHECK(pl.tail_b == tb_want);
  CHECK(pl.tail_t0 == (uint64_t)pl.nmain * pl.B);
  CHECK(pl.tail_t0 <= ntiles);
  CHECK(pl.nclaims == pl.nmain + cdiv(ntiles - pl.tail_t0, pl.tail_b));
  CHECK(pl.ntiles == ntiles);
  uint32_t next = 0;
  for (uint32_t c = 0; c < pl.nclaims; ++c) {
    const ClaimRange r = claim_range(pl, c);
    CHECK(r.tb == next);  // in order, no gap, no overlap
    CHECK(r.te > r.tb);   // non-empty
    CHECK(r.te <= ntiles);
    CHECK((r.tb & 1u) == 0);
    CHECK(r.te - r.tb <= 32);
    CHECK(r.te - r.tb == (c < pl.nmain ? pl.B : pl.tail_b) || c + 1 == pl.nclaims);
    CHECK(r.te - r.tb >= 2 || c + 1 == pl.nclaims);  // the kernels' claim loop: only the last may be one tile
    next = r.te;
  }
  CHECK(next == ntiles);
  for (uint32_t c : {pl.nclaims, pl.nclaims + 1, pl.nclaims + G, 0xFFFFFFFFu}) {
    const ClaimRange r = claim_range(pl, c);
    CHECK(r.tb == r.te);
  }
}

int main() {
  const uint32_t grids[] = {1, 2, 3, 7, 256, 1792};
  for (uint32_t G : grids) {
    for (uint32_t n = 0; n <= 6000; ++n) check(n, G);
    check(655360, G);
    check(65536, G);
  }
  {  // the 10 GiB build on 256 CUs x 7: batches of 32, the last 1792 of them in four claims each
    nt_ = 655360;
    G_ = 1792;
    const ClaimPlan pl = claim_plan(655360, 1792);
    CHECK(pl.B == 32 && pl.nmain == 18688);
    CHECK(pl.nclaims == 18688 + 1792 * CLAIM_TAIL_DIV);
    const ClaimPlan sm = claim_plan(5, 1792);  // fewer tiles than workgroups: claims of two, the last of one
    CHECK(sm.B == 2 && sm.nmain == 0 && sm.nclaims == 3);
  }
  if (failures) {
    printf("claim_test: %d checks failed\n", failures);
    return 1;
  }
  printf("claim_test ok (CLAIM_TAIL_DIV %d)\n", (int)CLAIM_TAIL_DIV);
  return 0;
}
