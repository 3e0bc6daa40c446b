// sidx_chunkwalk.hpp -- the arithmetic of the chunkrecord index's slab walk
// (shockidx_chunkrecord_fd_walk, sidx_walks.cpp; the slab step: shockidx_chunkrecord_slab_device)
// that needs no device: where slab k lies in the file and in its slot, how many rows a slab can
// emit, what one slab's workspace may grow to, how large a slab a device budget allows, and the
// precondition on a carry that enters a slab.  No HIP calls, so tests/host/chunkwalk_test.cpp
// exercises every piece on the CPU.
//
// Why the walk never submits a slab twice.  SeekChunk (fastq.go:216-243, fasta.go:143-173) reads
// only windows [w, w + WIN), and the walk over a view [lo, hi) that is not the file's last stops
// only at a window with w + WIN > hi, i.e. w > hi - WIN.  Slot k + 1 starts at lo' = hi - H (hi =
// (k + 1) S), so with H >= WIN: lo' <= hi - WIN < w -- the window the carry asks for next always
// lies in the next slot (chunkwalk_carry_enters), whatever the chunk size, however long the stretch
// without a match.  Windows only move forward, so nothing before lo' is ever needed again.
#pragma once
#include <stdint.h>

#include "sidx_common.hpp"
#include "sidx_slabwalk.hpp"  // largest_slab

namespace sidx {

constexpr u64 CHUNKWALK_WIN = 32768;             // SeekChunk's window (fastq.go:217, fasta.go:144)
constexpr u64 CHUNKWALK_HALO = 64ull << 10;      // H: bytes a slot keeps before its slab (>= WIN is all the carry needs)
constexpr u64 CHUNKWALK_PAD = 64;                // slot bytes past the readable ones (as the node buffer's)
constexpr u64 CHUNKWALK_ALIGN = 1ull << 20;      // slab bytes sized from a budget are a multiple of this
constexpr u64 CHUNKWALK_MIN_BUDGET = 32ull << 20;  // the smallest budget the sizing accepts (the column walk's)
constexpr u64 CHUNKWALK_MAX_SLAB = 1ull << 30;
constexpr u64 CHUNKWALK_CT = 16384;              // sidx_chunk.hip's position-table tile
static_assert(CHUNKWALK_HALO >= CHUNKWALK_WIN, "the window a walk stopped at lies in the next slot");
static_assert(CHUNKWALK_HALO % 16 == 0, "a slot's first byte is 16-byte aligned in the file for 16-byte-multiple slabs");

// Slot k of a walk with S-byte slabs over an n-byte file: file bytes [lo, hi) = [max(0, k S - H),
// min(n, (k + 1) S)), staged at the slot's first byte.  As a shockidx_slab: base = k S, front =
// base - lo, end = hi - base.
struct ChunkSlot {
  u64 lo, hi, base, front, end;
  bool first, last;  // lo == 0; hi == n
};
inline u64 chunkwalk_slots(u64 S, u64 n) { return n ? (n + S - 1) / S : 1; }
inline ChunkSlot chunkwalk_slot(u64 k, u64 S, u64 n) {
  ChunkSlot p;
  p.base = k * S < n ? k * S : n;
  p.lo = p.base < CHUNKWALK_HALO ? 0 : p.base - CHUNKWALK_HALO;
  p.hi = n - p.base < S ? n : p.base + S;
  p.front = p.base - p.lo;
  p.end = p.hi - p.base;
  p.first = p.lo == 0;
  p.last = p.hi == n;
  return p;
}
inline u64 chunkwalk_slot_bytes(u64 S) { return CHUNKWALK_HALO + S + CHUNKWALK_PAD; }

// The precondition on a carry entering a view that starts at lo: the open chunk's next window
// [off + chunk - WIN, ...) does not start before it.
inline bool chunkwalk_carry_enters(u64 off, u64 chunk, u64 lo) { return off + chunk - CHUNKWALK_WIN >= lo; }

// Rows one slab can emit over `span` bytes = hi - max(curr, lo): every chunk but the one that was
// open lies inside the span and is at least chunk - 32767 bytes long (a window's match ends at
// pos >= 1), plus the open chunk and, on the last slab, the EOF row.
inline u64 chunkwalk_row_bound(u64 span, u64 chunk) { return span / (chunk - 32767) + 2; }

// ---- one slab's workspace: what the speculative build of a `len`-byte view may hold ---------
// Node positions are predictions, so their tables are capped rather than grown: a view with more
// nodes than this predicts from the first ones only (FASTQ), or walks serially (FASTA).
inline u64 chunkwalk_nodes_cap(u64 len) { return len / 128 + 4096; }
// DevBuf::ensure's allocation for `need` elements of `elem` bytes
inline u64 chunkwalk_grown(u64 need, u64 elem) { return (need + need / 8 + 64) * elem; }
// c->d_cra: the FASTQ record table of the view behind node 0, or the FASTA tile counts, offsets and
// slots (gslot u16 per tile) with the scan's temporaries
inline u64 chunkwalk_cra_bytes(u64 len, u64 scan_bytes, u64 gslot) {
  const u64 fq = 16 * (chunkwalk_nodes_cap(len) + 1);
  const u64 nt = (len + CHUNKWALK_CT - 1) / CHUNKWALK_CT + 1;
  const u64 fa = 16 * nt + 2 * gslot * nt + scan_bytes + 2048;
  return fq > fa ? fq : fa;
}
// path rows of one round (as the whole-node build: about twice the chunk count)
inline u64 chunkwalk_path_cap(u64 len, u64 chunk) { return 2 * (len / chunk + 1) + 1024; }
// c->d_crb: node positions (FASTA), the position tiles, three jump tables over 3 nodes per FASTQ
// record, the path's heads, positions and results, the control words (each carved to 256 bytes)
inline u64 chunkwalk_crb_bytes(u64 len, u64 chunk) {
  const u64 nb = chunkwalk_nodes_cap(len) + 1, ntile = len / CHUNKWALK_CT + 2, cap = chunkwalk_path_cap(len, chunk);
  return 8 * nb + 8 * (ntile + 2) + 12 * 3 * nb + (4 + 8 + 8) * cap + 64 + 10 * 256;
}
// the tile block and the tile pass's staging of the view's FASTQ record index (run_index grows them
// with DevBuf::ensure; grid: the tile passes' persistent grid)
inline u64 chunkwalk_tile_bytes(u64 len, u64 grid) {
  const u64 nt = (len + TILE - 1) / TILE + 1, want = nt + nt / 8 + 64;
  const u64 block = (7 + 4 + 4) * 8 * want;
  const u64 stage = chunkwalk_grown((nt + grid + 16) * (u64)(TILE / 64), 4) + 64;
  const u64 words = chunkwalk_grown(nt * (u64)FQ_TILE_WORDS, 4) + 64;
  return block + stage + words;
}
struct ChunkWalkDev {  // what the sizing needs to know of the device side
  u64 carry_bytes, scan_bytes, gslot, grid;
};
// What a walk with S-byte slabs holds on the device: two slots, the carry, one slab's workspace
// (the view is S + H bytes) and one slab's rows.
inline u64 chunkwalk_footprint(u64 S, u64 chunk, const ChunkWalkDev &dv) {
  const u64 len = S + CHUNKWALK_HALO;
  return 2 * chunkwalk_slot_bytes(S) + dv.carry_bytes + chunkwalk_cra_bytes(len, dv.scan_bytes, dv.gslot) +
         chunkwalk_crb_bytes(len, chunk) + chunkwalk_tile_bytes(len, dv.grid) + 16 * chunkwalk_row_bound(len, chunk);
}
// The largest slab (a multiple of CHUNKWALK_ALIGN, at most 1 GiB) whose walk fits the budget; 0:
// the budget is under CHUNKWALK_MIN_BUDGET, or leaves no room for a slab.
inline u64 chunkwalk_slab_bytes(u64 budget, u64 chunk, const ChunkWalkDev &dv) {
  if (budget < CHUNKWALK_MIN_BUDGET) return 0;
  return largest_slab(CHUNKWALK_ALIGN, CHUNKWALK_MAX_SLAB, [&](u64 S) { return chunkwalk_footprint(S, chunk, dv) <= budget; });
}

// What the whole-node build of an n-byte node holds at its peak (shockidx_chunkrecord_fd without the
// walk): the node, its record table or tile arrays, the graph, the tile pass's words, the rows
// (DevBuf::ensure's growth included).
inline u64 chunkwalk_whole_bytes(u64 n, u64 chunk, const ChunkWalkDev &dv) {
  const u64 node = n + 64, rec = n / 128 + 4096;
  const u64 cra = chunkwalk_grown(chunkwalk_cra_bytes(n, dv.scan_bytes, dv.gslot) > 16 * rec
                                      ? chunkwalk_cra_bytes(n, dv.scan_bytes, dv.gslot) : 16 * rec, 1);
  const u64 crb = chunkwalk_grown(8 * rec + 8 * (n / CHUNKWALK_CT + 4) + 36 * rec + 20 * chunkwalk_path_cap(n, chunk) + 64 + 10 * 256, 1);
  return node + node / 8 + cra + crb + chunkwalk_tile_bytes(n, dv.grid) + chunkwalk_grown(chunkwalk_row_bound(n, chunk), 16) +
         (1ull << 20);
}

}  // namespace sidx
