// sidx_subwalk.hpp -- the arithmetic and decisions of the subset indexes' slab walk
// (shockidx_subset_fd_walk, sidx_walks.cpp) that need no device: how large an id slab and a
// parent window a device budget allows, which window follows a stop at an id, what a line that
// does not close means for the walk, and the row and run cursors.  No HIP calls, so
// tests/host/subwalk_test.cpp exercises every piece on the CPU.
#pragma once
#include <stdint.h>

#include "sidx_colwalk.hpp"  // the slot layout (colwalk_slab_at, COLWALK_FRONT, COLWALK_PAD)
#include "sidx_common.hpp"

namespace sidx {

constexpr u64 SUBWALK_HALO = 64ull << 10;         // id bytes readable past a slab
constexpr u64 SUBWALK_ALIGN = 4096;               // sized slabs are a multiple of this
constexpr u64 SUBWALK_MIN_BUDGET = 32ull << 20;   // the smallest budget the sizing accepts
constexpr u64 SUBWALK_MAX_SLAB = 256ull << 20;    // the largest id slab the sizing chooses

// A slab of S owned bytes consumes at most S / 2 + 1 ids (a non-blank line has two bytes at
// least), so tables of this many rows and runs are never short; the final run is the + 1 more.
inline u64 subwalk_rows_cap(u64 S) { return S / 2 + 2; }
inline u64 subwalk_runs_cap(u64 S) { return S / 2 + 3; }
inline u64 subwalk_slot_bytes(u64 S, u64 halo) { return colwalk_slot_bytes(S, halo); }

// The parent window of a budget: the whole index when a quarter of the budget holds it, else
// that quarter (at least one row).
inline u64 subwalk_window_rows(u64 budget, u64 parent_count) {
  const u64 w = budget / 4 / 16;
  const u64 r = parent_count < w ? parent_count : w;
  return r ? r : 1;
}

// What a walk with S-byte id slabs and W-row windows holds on the device: two id slots, the
// parent window, the carry and one call's workspace over a slab and its halo (ws(bytes): 8 bytes
// per text byte for the line ends and the per-line arrays for a line per byte at worst), one
// slab's rows and its runs.
template <class WsBytes>
u64 subwalk_footprint(u64 S, u64 halo, u64 W, u64 carry_bytes, WsBytes ws) {
  return 2 * subwalk_slot_bytes(S, halo) + 16 * W + carry_bytes + ws(S + halo) + 16 * subwalk_rows_cap(S) +
         16 * subwalk_runs_cap(S);
}
// The largest slab (a multiple of SUBWALK_ALIGN, at most SUBWALK_MAX_SLAB) whose walk fits the
// budget; 0: the budget is under SUBWALK_MIN_BUDGET, or the window and the halo leave no room.
template <class WsBytes>
u64 subwalk_slab_bytes(u64 budget, u64 halo, u64 W, u64 carry_bytes, WsBytes ws) {
  if (budget < SUBWALK_MIN_BUDGET) return 0;
  return largest_slab(SUBWALK_ALIGN, SUBWALK_MAX_SLAB, [&](u64 S) { return subwalk_footprint(S, halo, W, carry_bytes, ws) <= budget; });
}

// The window after a call stopped at id next_id (stop 2): it starts at that id's row, so a sparse
// list skips the rows between and a dense one goes on where the last window ended.
struct SubWindow {
  u64 row0, rows;
};
inline SubWindow subwalk_window_at(u64 row0, u64 W, u64 parent_count) {
  SubWindow w;
  w.row0 = row0 < parent_count ? row0 : parent_count;
  w.rows = parent_count - w.row0 < W ? parent_count - w.row0 : W;
  return w;
}
inline SubWindow subwalk_next_window(int64_t next_id, u64 W, u64 parent_count) {
  return subwalk_window_at((u64)next_id - 1, W, parent_count);  // (an id that stops is in [1, parent_count])
}

// A call that stopped at a line that does not close inside its window (stop 1): every line before
// next_off is consumed, so the next slab starts at that line in a fresh slot (Restart) -- unless
// the line heads this slab's slot already and still does not fit: no slot can hold it (NoMem:
// SHOCKIDX_ENOMEM, never a short table).
enum class SubRetry { Restart, NoMem };
inline SubRetry subwalk_on_open_line(u64 slab_lo, u64 next_off) {
  return next_off <= slab_lo ? SubRetry::NoMem : SubRetry::Restart;
}

// The two tables as they grow call by call: the next row / run number, and where the sinks write.
struct SubCursor {
  u64 rows = 0, runs = 0;
  u64 rows_pos() const { return 16 * rows; }
  u64 runs_pos() const { return 16 * runs; }
  u64 take_rows(u64 m) { const u64 at = rows; rows += m; return at; }
  u64 take_runs(u64 m) { const u64 at = runs; runs += m; return at; }
};

}  // namespace sidx
