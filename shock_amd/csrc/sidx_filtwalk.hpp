// sidx_filtwalk.hpp -- the arithmetic and decisions of the download filters' slab walk
// (shockidx_filter_fd_walk, sidx_walks.cpp; the slab step: shockidx_filter_slab_device) that need no
// device: where a slab lies, how many records a slab's view can hold, what one slab's workspace and
// output may grow to, how large a slab a device budget allows, which path shockidx_filter_fd takes,
// and what a slab's carried position means for the walk.  No HIP calls, so
// tests/host/filtwalk_test.cpp exercises every piece on the CPU.
#pragma once
#include <stdint.h>

#include "sidx_common.hpp"
#include "sidx_chunkwalk.hpp"  // chunkwalk_tile_bytes, chunkwalk_grown: the view's FASTQ record index
#include "sidx_colwalk.hpp"    // colwalk_default_halo
#include "sidx_slabwalk.hpp"   // largest_slab

namespace sidx {

constexpr u64 FILTWALK_PAD = 64;                  // slot / view bytes past the readable ones (as the node buffer's)
constexpr u64 FILTWALK_ALIGN = 64ull << 10;       // slab bytes sized from a budget are a multiple of this
constexpr u64 FILTWALK_MAX_SLAB = 1ull << 30;
constexpr u64 FILTWALK_MIN_BUDGET = 32ull << 20;  // the smallest budget the sizing accepts (as the other walks)
constexpr u64 FILTWALK_DETECT = 32768;            // bytes DetermineFormat reads (multi.go:43-62): the first slab holds them
// The shortest record GetReadOffset accepts (fastq.go:134-213): an id line of at least 3 bytes
// ("@", one ID byte, '\n': a 2-byte line is "missing sequence ID", :167-170), a sequence line of at
// least 2 (a 1-byte line is "empty sequence", :179-182), the plus line "+\n" (:191-194) and a
// quality line as long as the sequence line (:206-209) -- 9 bytes; the file's last record may lack
// its final '\n' (:202-205), which the + 1 below covers.
constexpr u64 FILTWALK_MIN_RECORD = 9;

inline u32 filtwalk_ndigits(u64 v) {  // fmt.Sprint(counter)'s length (anonymize.go:46)
  u32 d = 1;
  for (; v >= 10; v /= 10) ++d;
  return d;
}

// Slab [lo, lo + n) of an `size`-byte section: `end` readable bytes from its first byte (the slab
// and up to `halo` more), staged at its slot's first byte (front 0: no byte before the carried
// position is ever needed).  A slab whose window reaches the section's end is the last one and
// owns all of it.
struct FiltSlabPos {
  u64 lo, n, end;
  bool first, last;
};
inline FiltSlabPos filtwalk_slab_at(u64 lo, u64 S, u64 halo, u64 size, bool first) {
  FiltSlabPos p;
  p.lo = lo;
  p.n = size - lo < S ? size - lo : S;
  p.end = size - lo < p.n + halo ? size - lo : p.n + halo;
  p.first = first;
  p.last = lo + p.end == size;
  if (p.last) p.n = p.end;
  return p;
}
inline u64 filtwalk_slot_bytes(u64 S, u64 halo) { return S + halo + FILTWALK_PAD; }

// rows the record index of a `len`-byte view can hold (the row table is sized to it: no rerun)
inline u64 filtwalk_rows_cap(u64 len) { return len / FILTWALK_MIN_RECORD + 1; }
// Output bytes of `rows` records read from `len` input bytes, the largest counter max_counter.
// fq2fa writes ">" ID "\n" Seq "\n" (fasta.go:216-218): shorter than "@" ID "\n" Seq "\n" "+" ...;
// anonymize "@" counter "\n" Seq "\n+\n" Qual "\n" (fastq.go:283-285) replaces an ID of at least one
// byte by the counter's digits and the plus line by "+\n": at most digits - 1 bytes more per record.
inline u64 filtwalk_out_bound(u64 len, u64 rows, u64 max_counter) {
  return len + (u64)(filtwalk_ndigits(max_counter) - 1) * rows;
}
// the largest counter a section of `size` bytes can reach
inline u64 filtwalk_max_counter(u64 size) { return size / FILTWALK_MIN_RECORD + 1; }

// One slab call's carved workspace (c->d_sub) for K rows whose output is at most `out` bytes: the
// control words, spans (6 u32 per record), output lengths and offsets, the scan's temporaries and
// the first record of every output block (each piece rounded to 256 bytes: Carver).
inline u64 filtwalk_ws_bytes(u64 K, u64 out, u64 scan_bytes, u64 block) {
  auto r = [](u64 b) { return (b + 255) & ~255ull; };
  return r(64) + r(24 * (K + 1)) + 2 * r(8 * (K + 1)) + r(scan_bytes) + r(8 * (out / block + 4));
}

struct FiltWalkDev {  // what the sizing needs to know of the device side
  u64 carry_bytes, scan_bytes, block, grid;  // the scan's temporaries for the row cap; the writer's block; the tile grid
};
struct FiltWalkPlan {  // the exact-size buffers of a walk with S-byte slabs and a `halo`
  u64 slot, view, rows, ws, out;
};
inline FiltWalkPlan filtwalk_plan(u64 S, u64 halo, u64 size, const FiltWalkDev &dv) {
  const u64 len = S + halo, K = filtwalk_rows_cap(len);
  FiltWalkPlan p;
  p.slot = filtwalk_slot_bytes(S, halo);
  p.view = len + FILTWALK_PAD;
  p.rows = K > len / 32 + 4096 ? K : len / 32 + 4096;  // (never under what a record build starts with: it is not regrown)
  p.out = filtwalk_out_bound(len, K, filtwalk_max_counter(size)) + FILTWALK_PAD;
  p.ws = filtwalk_ws_bytes(K, p.out, dv.scan_bytes, dv.block);
  return p;
}
// What the walk holds on the device: two input slots, the view (the window from the carried
// position on, copied to a 16-byte-aligned address), the carry, one slab's rows, workspace and
// output, and the tile block of the view's record index.
inline u64 filtwalk_footprint(u64 S, u64 halo, u64 size, const FiltWalkDev &dv) {
  const FiltWalkPlan p = filtwalk_plan(S, halo, size, dv);
  return 2 * p.slot + p.view + dv.carry_bytes + 16 * p.rows + p.ws + p.out + chunkwalk_tile_bytes(S + halo, dv.grid) +
         2 * FILTWALK_DETECT;  // (the input staging still holds the bytes shockidx_filter_fd detected the format from)
}
// the halo a budget gets when the caller names none: the column walk's, and never more than a
// sixty-fourth of a small budget (a slab's buffers take about 14 bytes per window byte)
inline u64 filtwalk_default_halo(u64 budget) {
  const u64 h = colwalk_default_halo(budget), small = (budget / 64) & ~4095ull;
  return budget < (1ull << 30) && small < h ? small : h;
}
// The largest slab (a multiple of FILTWALK_ALIGN, at most 1 GiB) whose walk fits the budget; 0: the
// budget is under FILTWALK_MIN_BUDGET, or the halo leaves no room for a slab.
inline u64 filtwalk_slab_bytes(u64 budget, u64 halo, u64 size, const FiltWalkDev &dv) {
  if (budget < FILTWALK_MIN_BUDGET) return 0;
  return largest_slab(FILTWALK_ALIGN, FILTWALK_MAX_SLAB, [&](u64 S) { return filtwalk_footprint(S, halo, size, dv) <= budget; });
}

// What the whole path of shockidx_filter_fd holds at its peak over an n-byte FASTQ section, by the
// same worst case: the section, its rows, filter_section's workspace, the output and the tile block
// (DevBuf::ensure's growth included).
inline u64 filtwalk_whole_bytes(u64 n, const FiltWalkDev &dv) {
  const u64 K = filtwalk_rows_cap(n), out = filtwalk_out_bound(n, K, K) + FILTWALK_PAD;
  return chunkwalk_grown(n + FILTWALK_PAD, 1) + chunkwalk_grown(K, 16) +
         chunkwalk_grown(48 * (K + 8) + dv.scan_bytes + 8 * (out / dv.block + 4) + 4096, 1) + chunkwalk_grown(out, 1) +
         chunkwalk_tile_bytes(n, dv.grid) + chunkwalk_grown(3 * (n / TILE + 1) * (TILE / 64), 2);
}
// The same for anonymize over a FASTA or SAM section (not walked): records of 4 bytes at the least
// (">\nA\n" pieces, "\n"-separated lines), 72 bytes of rows and per-item arrays each, an output of
// at most three times the section (a counter of up to 8 digits for a 5-byte record).
inline u64 filtwalk_whole_other_bytes(u64 n, const FiltWalkDev &dv) {
  const u64 K = n / 4 + 4096;
  return chunkwalk_grown(n + FILTWALK_PAD, 1) + chunkwalk_grown(72 * K + dv.scan_bytes + 4096, 1) +
         chunkwalk_grown(3 * n + FILTWALK_PAD, 1) + chunkwalk_tile_bytes(n, dv.grid);
}

// What a slab's carried position means for the walk.  The slab [lo, ...) returned OK with the
// reader at pos, and the next slab was staged from `next_lo` on (front 0):
//   pos >= next_lo: the staged slab holds it (Continue);
//   pos <  next_lo: an owned record was not settled inside the halo -- the next slab starts at that
//                   record in a fresh slot (Restart), unless the record already heads this slab's
//                   slot (pos == lo): no slot can hold it (NoMem: SHOCKIDX_ENOMEM, never a short
//                   stream).
enum class FiltNext { Continue, Restart, NoMem };
inline FiltNext filtwalk_next(u64 lo, u64 next_lo, u64 pos) {
  if (pos >= next_lo) return FiltNext::Continue;
  return pos <= lo ? FiltNext::NoMem : FiltNext::Restart;
}

}  // namespace sidx
