// sidx_colwalk.hpp -- the arithmetic and decisions of the column index's slab walk
// (shockidx_column_fd_walk, sidx_walks.cpp) that need no device: how large a slab a device
// budget allows, where a slab lies in its slot, what a slab's result means for the walk (the one
// retry rule), and the row cursor.  No HIP calls, so tests/host/colwalk_test.cpp exercises every
// piece on the CPU.
#pragma once
#include <stdint.h>

#include "sidx_common.hpp"
#include "sidx_slabwalk.hpp"  // largest_slab

namespace sidx {

constexpr u64 COLWALK_FRONT = 16;             // bytes a slot keeps before a slab that does not start the file
constexpr u64 COLWALK_PAD = 64;               // slot bytes past the readable ones (as the node buffer's)
constexpr u64 COLWALK_HALO = 4ull << 20;      // bytes readable past a slab, unless the budget is small
constexpr u64 COLWALK_ALIGN = 1ull << 20;     // slab bytes are a multiple of this (and so of the tile)
constexpr u64 COLWALK_MIN_BUDGET = 32ull << 20;  // the smallest budget the sizing accepts
static_assert(COLWALK_ALIGN % TILE == 0, "slabs are whole tiles");

// rows a slab's table starts with (16 bytes per 32 input bytes, as the other walks; grown on ESPACE)
inline u64 colwalk_rows_cap(u64 S) { return S / 32 + 4096; }
// one input slot: [front | slab | halo | pad]
inline u64 colwalk_slot_bytes(u64 S, u64 halo) { return COLWALK_FRONT + S + halo + COLWALK_PAD; }
// the halo a budget gets when the caller names none: 4 MiB, a sixteenth of a small budget
inline u64 colwalk_default_halo(u64 budget) {
  const u64 h = (budget / 16) & ~4095ull;
  return h < COLWALK_HALO ? h : COLWALK_HALO;
}
// What a walk with S-byte slabs holds on the device: two input slots, the carry and one slab's
// column workspace (ws(tiles): sidx_col_tile_bytes) and its rows.
template <class WsBytes>
u64 colwalk_footprint(u64 S, u64 halo, u64 carry_bytes, WsBytes ws) {
  return 2 * colwalk_slot_bytes(S, halo) + carry_bytes + ws((S + TILE - 1) / TILE) + 16 * colwalk_rows_cap(S);
}
// The largest slab (a multiple of COLWALK_ALIGN, at most 1 GiB) whose walk fits the budget; 0: the
// budget is under COLWALK_MIN_BUDGET, or the halo leaves no room for a slab.
template <class WsBytes>
u64 colwalk_slab_bytes(u64 budget, u64 halo, u64 carry_bytes, WsBytes ws) {
  if (budget < COLWALK_MIN_BUDGET) return 0;
  return largest_slab(COLWALK_ALIGN, 1ull << 30, [&](u64 S) { return colwalk_footprint(S, halo, carry_bytes, ws) <= budget; });
}

// Slab [lo, lo + n) of a size-byte file in its slot: `front` bytes before it and `end` readable
// bytes from its first byte on (the slab and up to `halo` more); the slot's byte 0 is file byte
// lo - front, so the slab's first byte sits 16-byte aligned at COLWALK_FRONT for every slab but
// the file's first (front 0: at 0).
struct ColSlabPos {
  u64 lo, n, end, front;
  bool first, last;  // it starts the file; its owned bytes end it
};
inline ColSlabPos colwalk_slab_at(u64 lo, u64 S, u64 halo, u64 size) {
  ColSlabPos p;
  p.lo = lo;
  p.n = size - lo < S ? size - lo : S;
  p.end = size - lo < p.n + halo ? size - lo : p.n + halo;
  p.front = lo < COLWALK_FRONT ? 0 : COLWALK_FRONT;  // (a slab that starts inside the file's first 16 bytes reads none before it)
  p.first = lo == 0;
  p.last = lo + p.n == size;
  return p;
}
// the slab shortened to m owned bytes (the retry rule): it keeps its window's start and its halo
inline ColSlabPos colwalk_shorten(const ColSlabPos &p, u64 m, u64 halo, u64 size) {
  ColSlabPos q = colwalk_slab_at(p.lo, m, halo, size);
  q.front = p.front;
  return q;
}

// The one retry rule.  A slab that returned SHOCKIDX_EMORE with state_out = the file offset x of the
// first owned line it could not settle: that line follows the '\n' at x - 1, so
//   x - 1 > lo:  the slab is submitted again as [lo, x - 1) -- it no longer owns the line -- and the
//                next slab starts at x - 1 in a fresh slot (Shorten, *cut = x - 1);
//   otherwise:   the line heads a slot (or the file) and still does not fit: no slot can hold it
//                (NoMem: SHOCKIDX_ENOMEM, never a short table).
enum class ColRetry { Shorten, NoMem };
inline ColRetry colwalk_on_more(u64 lo, u64 state_out, u64 *cut) {
  if (state_out == 0 || state_out - 1 <= lo) return ColRetry::NoMem;
  *cut = state_out - 1;
  return ColRetry::Shorten;
}
// SHOCKIDX_ESPACE with `need` rows: the capacity to submit the slab again with
inline u64 colwalk_grow_rows(u64 cap, u64 need) {
  const u64 g = need + need / 8 + 64;
  return g > cap ? g : cap + 1;
}

// The table as it grows slab by slab: the rows so far and where the sink writes the next ones.
struct ColRowCursor {
  u64 total = 0;
  u64 file_pos() const { return 16 * total; }  // the .idx byte the next row goes to
  u64 take(u64 m) {                            // m more rows: their first row number
    const u64 at = total;
    total += m;
    return at;
  }
};

}  // namespace sidx
