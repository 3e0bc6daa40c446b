// sidx_slabwalk.hpp -- the arithmetic and decisions of the slab pipelines (sidx_pipeline.cpp)
// that need no device: where the slabs lie, what a slab's device result means for the walk,
// how the row table continues from slab to slab, and where it must end.  No HIP calls, so
// tests/host/slabwalk_test.cpp exercises every piece on the CPU.
#pragma once
#include <stdint.h>

#include "sidx_common.hpp"

namespace sidx {

constexpr u64 PIPE_SLAB = 1ull << 30;    // slab bytes (the ring's slabs are sized to the budget)
constexpr u64 PIPE_HALO = 4ull << 20;    // bytes readable past a slab (records crossing its end)
constexpr u64 RING_FRONT = 64ull << 10;  // ring layout: bytes kept in the slot before a slab

// Slab k of an n-byte node cut into S-byte slabs: file bytes [lo, lo + len) owned,
// [lo, lo + end) readable, front bytes readable before it (whole layout: everything before it,
// the node is in one buffer; ring layout: what the slot holds).
struct SlabLayout {
  u64 n, S;
  bool ring;
  u64 count() const { return (n + S - 1) / S; }
  u64 lo(u64 k) const { return k * S; }
  u64 len(u64 k) const { return n - lo(k) < S ? n - lo(k) : S; }
  u64 end(u64 k) const { return n - lo(k) < len(k) + PIPE_HALO ? n - lo(k) : len(k) + PIPE_HALO; }
  u64 front(u64 k) const { return ring ? (lo(k) < RING_FRONT ? lo(k) : RING_FRONT) : lo(k); }
  bool eof(u64 k) const { return lo(k) + end(k) == n; }   // the readable bytes reach the node's end
  bool last(u64 k) const { return lo(k) + len(k) == n; }  // the owned bytes do
};

// Ring layout: the slab bytes that two slots and one slab's workspaces leave of a device budget
// (rows 16 B per 32 input bytes, tile words and starts ~1/16, status ~1/40: ~0.6 S; 2.7 S in
// all), a multiple of 16 MiB, at most PIPE_SLAB.  0: the budget is too small (under 64 MiB slabs).
constexpr u64 RING_FIXED = 2 * (RING_FRONT + PIPE_HALO + 64) + (96ull << 20), RING_MIN_SLAB = 64ull << 20,
              RING_SLAB_ALIGN = 16ull << 20;
inline u64 ring_slab_bytes(u64 budget) {
  u64 S = budget > RING_FIXED ? (budget - RING_FIXED) * 10 / 27 : 0;
  S = S > PIPE_SLAB ? PIPE_SLAB : S & ~(RING_SLAB_ALIGN - 1);
  return S < RING_MIN_SLAB ? 0 : S;
}

// The sizing of the carried-state walks (sidx_colwalk.hpp, sidx_subwalk.hpp, sidx_chunkwalk.hpp):
// the largest multiple of `align`, at most `max`, whose footprint fits(S) the budget; 0: none
// does.  A footprint grows with S, so fits holds up to some S and fails above it: a bisection on
// S / align.
template <class Fits>
u64 largest_slab(u64 align, u64 max, Fits fits) {
  u64 lo = 0, hi = max / align;
  while (lo < hi) {
    const u64 mid = (lo + hi + 1) / 2;
    if (fits(mid * align)) lo = mid;
    else hi = mid - 1;
  }
  return lo * align;
}

// What a slab's index pass (run_index's code rc, its device result) means for the walk.
enum class SlabOutcome {
  Clean,     // its rows continue the table, on to the next slab
  GoError,   // ring: a Go format error inside a slab indexed with its exact incoming state is the
             //   file's first (the slabs before it were clean) -- its rows before the error and
             //   its text end the build, as the one-pass build ends them (record.go:51-83)
  Partial,   // ring: a record the slab could not close through its halo (ST_NEEDMORE) or blank
             //   lines running past it (ST_END before the file's end): the rows before it are
             //   final too, and the walk restarts at it
  FallBack,  // anything else (a device flag, a short count, an error in the whole layout): the
             //   slab's rows are not used
};
inline SlabOutcome classify(int rc, const DevResult &dr, u64 row_base, bool last, bool ring) {
  const bool counted = rc == 0 && dr.count >= row_base;
  const bool ok = counted && dr.flags == 0;
  if (ok && (dr.code == ST_OK || (last && (dr.code == ST_END || dr.code == ST_ABSENT)))) return SlabOutcome::Clean;
  if (!ring) return SlabOutcome::FallBack;
  if (ok && dr.code >= ST_FQ_TRUNC && dr.code <= ST_FA_INVALID && (dr.code != ST_FQ_TRUNC || last))
    return SlabOutcome::GoError;
  if (counted && !last && ((dr.flags == RF_HALO && dr.code == ST_NEEDMORE) || (dr.flags == 0 && dr.code == ST_END)))
    return SlabOutcome::Partial;
  return SlabOutcome::FallBack;
}

// The row table as it grows slab by slab (record.go:51-83: row i + 1 starts where row i ends).
struct RowCursor {
  u64 total;     // rows so far
  u64 next_off;  // where the next row must start
  u64 last_len;  // the last row's length
  // m rows ({offset, length} pairs) continue the table.  false: a slab's first row does not start
  // where the previous slab's rows end (only a slab's first chunk is checked; nothing advances).
  bool accept(const u64 *rows, u64 m, bool first_chunk_of_slab) {
    if (!m) return true;
    if (first_chunk_of_slab && rows[0] != next_off) return false;
    last_len = rows[2 * (m - 1) + 1];
    next_off = rows[2 * (m - 1)] + last_len;
    total += m;
    return true;
  }
};

// End-of-table invariant of a clean walk: the rows end where the file does (`end`) -- FASTQ: or
// before trailing blank lines (fastq.go:141-156) -- and a line table's last row, the bytes after
// the last '\n' (line.go:37-45), is empty when the file ends in '\n'.  byte_at(off, &b) reads one
// file byte; a failed read counts as a violation.
template <class ByteAt>
bool table_ends_at_file_end(int kfmt, u64 next_off, u64 end, u64 last_len, ByteAt byte_at) {
  uint8_t a = 0, z = 0;
  if (next_off > end) return false;
  if (next_off < end &&
      (kfmt != F_FASTQ || !byte_at(next_off, &a) || !byte_at(end - 1, &z) || a != '\n' || z != '\n'))
    return false;
  if (kfmt == F_LINE && last_len) return byte_at(end - 1, &z) && z != '\n';
  return true;
}

}  // namespace sidx
