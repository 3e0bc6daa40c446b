// sidx_batch_host.hpp -- the pure arithmetic of the batch build (sidx_batch_api.cpp,
// sidx_batch.hip): which {pos, len} a batch accepts, how the host entry point packs node bodies
// into one arena, the small-node limit, a single node's row region and how a list splits into
// batched nodes and singles.  No HIP call and no allocation, so tests/host/batch_test.cpp runs it
// on the CPU; batch_node_ok is also the range check the classify kernel makes.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#define SIDX_BATCH_HD __host__ __device__
#else
#define SIDX_BATCH_HD
#endif

namespace sidx {

constexpr uint64_t BATCH_ALIGN = 16;  // a node starts on a 16-byte boundary of the arena (one lane load)

// A node of the list lies inside the arena, 16-byte aligned, with no overflow in pos + len.
SIDX_BATCH_HD inline bool batch_node_ok(int64_t pos, int64_t len, uint64_t data_len) {
  return pos >= 0 && len >= 0 && ((uint64_t)pos & (BATCH_ALIGN - 1)) == 0 && (uint64_t)pos <= data_len &&
         (uint64_t)len <= data_len - (uint64_t)pos;
}

// small: at most `limit` bytes, and a limit of 0 sends every node through the single build
SIDX_BATCH_HD inline bool batch_is_small(uint64_t len, uint64_t limit) { return limit != 0 && len <= limit; }

// Positions of K bodies packed back to back, each at the next 16-byte boundary; *arena_len = the
// arena's bytes (a multiple of 16).  False when the total does not fit 63 bits (a position is an int64).
inline bool batch_pack(const uint64_t *lens, uint64_t K, uint64_t *pos, uint64_t *arena_len) {
  constexpr uint64_t LIM = (1ull << 63) - BATCH_ALIGN;
  uint64_t off = 0;
  for (uint64_t i = 0; i < K; ++i) {
    pos[i] = off;
    if (lens[i] > LIM - off) return false;
    off = (off + lens[i] + BATCH_ALIGN - 1) & ~(BATCH_ALIGN - 1);
  }
  *arena_len = off;
  return true;
}

// SHOCKIDX_BATCH_SMALL: a decimal byte count; unset, empty or not a number: the default
inline uint64_t batch_small_limit(const char *env, uint64_t dflt) {
  if (!env || !*env) return dflt;
  char *end = nullptr;
  const unsigned long long v = strtoull(env, &end, 10);
  return end != env ? (uint64_t)v : dflt;
}

// Rows a table of `total` rows leaves a node whose region starts at row_off, the next node's at
// next_off (total for the last node): what a single build may write.  0 for an inconsistent layout.
inline uint64_t batch_region_rows(uint64_t row_off, uint64_t next_off, uint64_t total) {
  return row_off <= next_off && next_off <= total ? next_off - row_off : 0;
}

// The host entry point's first row capacity for an arena: a row per 16 bytes and two per node
// (a line index of short lines needs more: the call then reports what it needs and is repeated).
// False on overflow of the byte size 16 * rows.
inline bool batch_rows_guess(uint64_t arena_len, uint64_t K, uint64_t *rows) {
  if (K > (1ull << 58)) return false;
  const uint64_t r = arena_len / 16 + 2 * K + 64;
  if (r > (1ull << 59)) return false;
  *rows = r;
  return true;
}

// How a list of K nodes splits when `singles` of them are too long for the batched walk.
struct BatchSplit {
  uint64_t batches, batched, singles;
};
inline bool batch_split(uint64_t K, uint64_t singles, BatchSplit *out) {
  if (singles > K) return false;
  out->singles = singles;
  out->batched = K - singles;
  out->batches = out->batched ? 1 : 0;  // every small node, whatever its format, in one batch
  return true;
}

}  // namespace sidx
