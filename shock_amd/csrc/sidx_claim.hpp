// sidx_claim.hpp -- which tiles a workgroup of a persistent tile pass takes (k_fq_tiles,
// k_fa_tiles): the tiles are cut into claims, numbered in file order, and the workgroups take
// them in that order (the first G by block index, every later one by a device counter), so a
// workgroup that runs slower simply takes fewer.  Pure integer code with no HIP call, shared by the
// kernels and the CPU test (tests/host/claim_test.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SIDX_CLAIM_HD __host__ __device__ inline
#else
#define SIDX_CLAIM_HD inline
#endif

namespace sidx {

// The last G batches are handed out in claims of B / CLAIM_TAIL_DIV tiles (1: whole batches to
// the end), so the workgroups' last claims end closer together.
#ifndef CLAIM_TAIL_DIV
#define CLAIM_TAIL_DIV 2
#endif
static_assert(CLAIM_TAIL_DIV == 1 || CLAIM_TAIL_DIV == 2 || CLAIM_TAIL_DIV == 4, "the tail's claims: B, B/2 or B/4 tiles");
constexpr uint32_t CLAIM_BMAX = 32;  // tiles per batch of a large input (the measured best, DESIGN.md §3 "Tile order")
constexpr uint32_t CLAIM_BMIN = 2;   // every claim starts at an even tile

struct ClaimPlan {
  uint32_t B;        // tiles per claim of the main part
  uint32_t nmain;    // claims of B tiles: every batch but the last G
  uint32_t tail_b;   // tiles per claim of the tail
  uint32_t tail_t0;  // first tile of the tail
  uint32_t nclaims;  // claims in all; claim c covers claim_range(plan, c)
  uint32_t ntiles;
};
struct ClaimRange {
  uint32_t tb, te;  // tiles [tb, te)
};

// The plan for ntiles tiles on a grid of G workgroups.  B is the largest of 32, 16, 8, 4, 2 that
// still leaves every workgroup four batches or more (a small input spreads over the whole grid
// and its last round is short), else 2.
SIDX_CLAIM_HD ClaimPlan claim_plan(uint32_t ntiles, uint32_t G) {
  uint32_t B = CLAIM_BMAX;
  while (B > CLAIM_BMIN && (uint64_t)((ntiles + B - 1) / B) < 4ull * G) B >>= 1;
  const uint32_t nb = (ntiles + B - 1) / B;
  ClaimPlan pl;
  pl.B = B;
  pl.nmain = nb > G ? nb - G : 0u;
  pl.tail_b = B / CLAIM_TAIL_DIV > CLAIM_BMIN ? B / CLAIM_TAIL_DIV : CLAIM_BMIN;
  pl.tail_t0 = pl.nmain * B;  // (< ntiles: nmain < nb)
  pl.nclaims = pl.nmain + (ntiles - pl.tail_t0 + pl.tail_b - 1) / pl.tail_b;
  pl.ntiles = ntiles;
  return pl;
}

// The tiles of claim c; empty (tb == te) from c = nclaims on.  Every tb is even, and no claim but
// the last is shorter than two tiles.
SIDX_CLAIM_HD ClaimRange claim_range(const ClaimPlan &pl, uint32_t c) {
  ClaimRange r;
  if (c < pl.nmain) {
    r.tb = c * pl.B;
    r.te = r.tb + pl.B;
  } else if (c < pl.nclaims) {
    r.tb = pl.tail_t0 + (c - pl.nmain) * pl.tail_b;
    r.te = pl.ntiles - r.tb > pl.tail_b ? r.tb + pl.tail_b : pl.ntiles;
  } else {
    r.tb = r.te = pl.ntiles;
  }
  return r;
}

}  // namespace sidx
