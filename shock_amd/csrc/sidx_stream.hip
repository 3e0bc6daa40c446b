// sidx_stream.hip -- gfx950 kernels of the sectioned download stream: request.Streamer.Stream with a
// Filter (request/streamer.go:78-98) over a list of sections {int64 pos, int64 len} of one node in
// HBM.  The reference builds a new filter reader per section (s.Filter(sr), streamer.go:86-87), so
// fastq.Reader.Read (fastq.go:50-132) restarts at every section and a section's end is its reader's
// end of file.  What is here is the segmented index over many small sections -- FASTQ records, and
// under anonymize (which detects the format per section) FASTA sequences and SAM lines, further down;
// spans, scan and writer are the single-section filter's (sidx_filter.hip), on absolute positions of the
// node.
//
// A section's records are fixed by its '\n' ranks alone.  Read consumes four lines per record and
// returns at the first record it cannot deliver; a blank first line never starts a record (the
// skip-blank loop, :59-68, ends in io.EOF or in "empty line(s) between records").  So record k of a
// section is its lines 4k .. 4k + 3, the records can be checked independently, and the first one that
// fails ends the section's stream; what follows the last whole group of four lines (the tail) gives
// the section's terminal status: nothing or blank lines (io.EOF), a record whose quality line has no
// '\n' (returned with io.EOF, dropped by the filters), or Read's error.
//
//   k_ss_classify  one lane per section: range check; which sections the segmented path cannot take, and
//                  where a batch (a run of consecutive small sections of one format) starts
//   k_ss_count     one wave per section: its '\n' count / 4 = the records that have all four line ends
//   (exclusive scan over the sections, sidx_scan.hpp)
//   k_ss_emit      one wave per section: the flat row table, each record's ordinal in its section and
//                  its section; the tail's status through fastq_read_status over a wave accessor that
//                  ends at the section end
//   k_ss_check     one lane per record: Read's checks in Read's order (fastq_read_status over the
//                  record's four known line ends)
//   k_ss_finish    the first failing (section, record, status) -> the number of records delivered
//
// A wave per section, 16 bytes per lane and step, '\n' masks ranked by a wave scan.  Sections of a few
// hundred bytes leave two thirds of the lanes idle in the one step they take; they do not share a
// wave: the pass is bound by the latency of one round of loads per section, a workgroup's four waves
// hold four sections in flight with no LDS and few registers, so the CU's wave slots (not its lanes)
// are what hides that latency, and a shared wave would add a segmented rank per lane group for the
// same number of loads in flight.
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"
#include "sidx_device.hpp"
#include "sidx_fastq_read.hpp"
#include "sidx_launch.hpp"
#include "sidx_seg.hpp"
#include "sidx_stream.hpp"

namespace sidx {

__device__ __forceinline__ bool sec_valid(i64 pos, i64 len, u64 n) {
  return pos >= 0 && len >= 0 && (u64)pos <= n && (u64)len <= n - (u64)pos;
}

// The small-section limits by format (bytes; 0: that format takes the single-section path).
struct SmallLimits { u64 fastq, fasta, sam; };

// The format the segmented path takes section i in, 0: it does not (outside the node, too long, or of
// no detected format).  fmt null: fq2fa, which does not detect and reads everything as FASTQ.
__device__ __forceinline__ int ss_batched(const i64 *secs, u64 i, u64 n, const int *fmt, const SmallLimits &sm) {
  const i64 pos = secs[2 * i], len = secs[2 * i + 1];
  if (!sec_valid(pos, len, n)) return 0;
  const int f = fmt ? fmt[i] : (int)F_FASTQ;
  const u64 lim = f == F_FASTQ ? sm.fastq : f == F_FASTA ? sm.fasta : f == F_SAM ? sm.sam : 0;
  return (u64)len <= lim && lim ? f : 0;
}

// fmt: the sections' detected formats (anonymize; null for fq2fa, which does not detect,
// fq2fa.go:18-24).  ctl[SS_INVALID] |= 1 for a section outside the node; a section longer than its
// format's limit or of no format is appended to others (any order; the host sorts them), counted in
// ctl[SS_NOTHER].  A batch is a maximal run of consecutive sections the segmented path takes in one
// format: every section after the first that starts one -- its predecessor is an other or of another
// format -- is appended to cuts with its format (any order), counted in ctl[SS_NCUT]; section 0's
// format goes to ctl[SS_FMT0].  A list of small sections of one format reports no other and no cut.
__global__ __launch_bounds__(256) void k_ss_classify(const i64 *secs, u64 nsecs, u64 n, const int *fmt, SmallLimits sm,
                                                     u64 *ctl, u64 *others, u64 *cuts) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsecs) return;
  const i64 pos = secs[2 * i], len = secs[2 * i + 1];
  if (!sec_valid(pos, len, n)) {
    atomicOr((unsigned long long *)&ctl[SS_INVALID], 1ull);
    return;
  }
  const int f = ss_batched(secs, i, n, fmt, sm);
  if (!f) {
    const u64 k = atomicAdd((unsigned long long *)&ctl[SS_NOTHER], 1ull);
    others[k] = i;  // at most nsecs entries
    return;
  }
  if (i == 0) {
    ctl[SS_FMT0] = (u64)f;
  } else if (ss_batched(secs, i - 1, n, fmt, sm) != f) {
    const u64 k = atomicAdd((unsigned long long *)&ctl[SS_NCUT], 1ull);
    cuts[k] = (i << SS_CUT_SHIFT) | (u64)f;  // at most nsecs entries
  }
}

// The 16 bytes of lane `lane` in the 1 KiB step at b0 (16-byte aligned) and their '\n' mask inside
// [pos, end); a: the chunk's position.  end <= n, so a chunk below end starts inside the node.
__device__ __forceinline__ u32 ss_nl_mask(const uint8_t *data, u64 n, u64 b0, int lane, u64 pos, u64 end, u64 &a) {
  a = b0 + 16ull * lane;
  if (a >= end) return 0;
  const uint4 v = (a + 16 <= n) ? load16(data + a) : load16_partial(data, a, n);
  u32 m = eq16(v, '\n');
  if (a < pos) m &= ~0u << (u32)(pos - a);
  if (end - a < 16) m &= (1u << (u32)(end - a)) - 1u;
  return m;
}

__device__ __forceinline__ u64 ss_wave_max(u64 v) {
  for (int o = 32; o > 0; o >>= 1) {
    const u64 y = __shfl_xor(v, o, 64);
    v = v > y ? v : y;
  }
  return v;
}

// shift 2: FASTQ records (four lines each); shift 0: SAM lines
__global__ __launch_bounds__(256) void k_ss_count(const uint8_t *data, u64 n, const i64 *secs, u64 S, u64 *cnt,
                                                  u32 shift) {
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 i = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < S; i += nw) {
    const u64 pos = (u64)secs[2 * i], end = pos + (u64)secs[2 * i + 1];
    u32 c = 0;
    for (u64 b0 = pos & ~15ull; b0 < end; b0 += 1024) {
      u64 a;
      c += (u32)__builtin_popcount(ss_nl_mask(data, n, b0, lane, pos, end, a));
    }
    u64 t = c;
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) cnt[i] = t >> shift;
  }
}

// rows[2 r] = record r's start, rows[2 r + 1] = its END (k_ss_check turns it into the length);
// ord[r] = its ordinal within its section, rsec[r] = its section (relative to the batch).
__global__ __launch_bounds__(256) void k_ss_emit(const uint8_t *data, u64 n, const i64 *secs, u64 S, const u64 *cnt,
                                                 const u64 *base, u64 *rows, u32 *ord, u32 *rsec, u64 *ctl) {
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 i = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < S; i += nw) {
    const u64 pos = (u64)secs[2 * i], end = pos + (u64)secs[2 * i + 1];
    const u64 nfull = cnt[i], r0 = base[i];
    u64 tail = pos;  // where the reader stands after the last whole record
    if (nfull) {
      if (lane == 0) rows[2 * r0] = pos;
      u64 rank0 = 0;  // '\n' before this step
      for (u64 b0 = pos & ~15ull; b0 < end && rank0 < 4 * nfull; b0 += 1024) {
        u64 a;
        u32 m = ss_nl_mask(data, n, b0, lane, pos, end, a);
        const u32 c = (u32)__builtin_popcount(m);
        const u32 incl = wave_scan_add(c);
        u64 q = rank0 + incl - c;
        for (; m; m &= m - 1, ++q) {
          if ((q & 3) != 3) continue;
          const u64 k = q >> 2;
          if (k >= nfull) break;
          const u64 e = a + (u64)__builtin_ctz(m) + 1;
          rows[2 * (r0 + k) + 1] = e;
          ord[r0 + k] = (u32)k;
          rsec[r0 + k] = (u32)i;
          if (k + 1 < nfull) rows[2 * (r0 + k + 1)] = e;
          else tail = e;
        }
        rank0 += (u32)__shfl((int)incl, 63, 64);
      }
      tail = ss_wave_max(tail);
    }
    WaveAcc wa;
    wa.g = data; wa.end = end; wa.eof = 1; wa.lane = lane; wa.front = 0;
    // fewer than four '\n' are left, so ST_OK here is the record Read returns with io.EOF: dropped
    const u32 st = fastq_read_status(wa, tail);
    if (lane == 0 && st != ST_OK && st != ST_END)
      atomicMin((unsigned long long *)&ctl[SS_KEY], (unsigned long long)ss_key(i, nfull, st));
  }
}

// One record's view for fastq_read_status: its four line ends are known (e3 = the record's last
// byte), so Read's ReadBytes('\n') calls are answered from them; only the skip-blank loop of a record
// that starts on a blank line walks bytes, up to the section end.
struct RecAcc {
  const uint8_t *g;
  u64 end;  // the section end
  u64 e0, e1, e2, e3;
  __device__ __forceinline__ u32 byte(u64 p) const { return g[p]; }
  __device__ __forceinline__ const uint8_t *ptr() const { return g; }
  __device__ __forceinline__ u64 base() const { return 0; }
  __device__ u32 find(int cls, u64 p, u64 /*lim*/, u64 &out) const {
    if (cls == C_NL) {
      if (p <= e0) { out = e0; return FR_FOUND; }
      if (p <= e1) { out = e1; return FR_FOUND; }
      if (p <= e2) { out = e2; return FR_FOUND; }
      if (p <= e3) { out = e3; return FR_FOUND; }
      for (; p < end; ++p)
        if (g[p] == '\n') { out = p; return FR_FOUND; }
      return FR_NONE;
    }
    for (; p < end; ++p)  // C_NOTNL
      if (g[p] != '\n') { out = p; return FR_FOUND; }
    return FR_NONE;
  }
};

__global__ __launch_bounds__(256) void k_ss_check(const uint8_t *data, u64 n, const i64 *secs, u64 *rows, const u32 *ord,
                                                  const u32 *rsec, u64 K, u64 *ctl) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= K) return;
  const u64 off = rows[2 * r], end = rows[2 * r + 1];
  rows[2 * r + 1] = end - off;
  const u64 i = rsec[r];
  RecAcc ra;
  ra.g = data;
  ra.end = (u64)secs[2 * i] + (u64)secs[2 * i + 1];
  ra.e0 = ra.e1 = ra.e2 = 0;
  ra.e3 = end - 1;
  first3_nl(data, n, off, end, ra.e0, ra.e1, ra.e2);
  const u32 st = fastq_read_status(ra, off);
  if (st != ST_OK) atomicMin((unsigned long long *)&ctl[SS_KEY], (unsigned long long)ss_key(i, ord[r], st));
}

__global__ void k_ss_finish(const u64 *base, u64 K, u64 *ctl) {
  if (threadIdx.x || blockIdx.x) return;
  const u64 key = ctl[SS_KEY];
  ctl[SS_KE] = key == ~0ull ? K : base[key >> SS_SEC_SHIFT] + ((key >> 4) & SS_REC_MASK);
}

// ---- FASTA and SAM sections (anonymize) --------------------------------------------------------------
// fasta.Reader.Read's sequences in a section are cut at the section's FASTA boundaries: a '>' at p whose
// last '\n' in [pos, p) lies after the last '>' in [pos, p) (fasta.go:100-138, over the section's bytes
// alone: its first '>' is never a boundary, whatever precedes it in the node).  Sequence k is the read
// [start_k, B_k), start_0 = pos, start_k = B_{k-1}; the read that runs to the section end comes back with
// io.EOF and is dropped (fasta.go:86-88), so a section has no terminal status and the first failing
// sequence in flat order is the first failure of the stream.  sam.Reader.Read's items are the section's
// '\n'-terminated lines; a last piece without '\n' is io.EOF and delivers nothing (sam.go:49,72-74).
//
//   k_ss_fa_count  one wave per section: its boundaries
//   k_ss_fa_emit   the flat row table (start, B_k), each sequence's ordinal in its section and its section
//   k_ss_count     (shift 0) a section's '\n'
//   k_ss_sam_emit  the flat row table (offset, length) of the lines, and each line's section
//   k_ss_flat_finish  the first failing flat item -> its section, the items before it, the lines delivered
// Spans and writers are sidx_filter.hip's, over the flat rows.

// ss_nl_mask for the two byte classes of the boundary rule
__device__ __forceinline__ void ss_nl_gt_masks(const uint8_t *data, u64 n, u64 b0, int lane, u64 pos, u64 end, u64 &a,
                                               u32 &mnl, u32 &mgt) {
  a = b0 + 16ull * lane;
  mnl = mgt = 0;
  if (a >= end) return;
  const uint4 v = (a + 16 <= n) ? load16(data + a) : load16_partial(data, a, n);
  u32 keep = 0xFFFFu;
  if (a < pos) keep &= ~0u << (u32)(pos - a);
  if (end - a < 16) keep &= (1u << (u32)(end - a)) - 1u;
  mnl = eq16(v, '\n') & keep;
  mgt = eq16(v, '>') & keep;
}

__global__ __launch_bounds__(256) void k_ss_fa_count(const uint8_t *data, u64 n, const i64 *secs, u64 S, u64 *cnt) {
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 i = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < S; i += nw) {
    const u64 pos = (u64)secs[2 * i], end = pos + (u64)secs[2 * i + 1];
    u64 cnl = 0, cgt = 0;
    u32 c = 0;
    for (u64 b0 = pos & ~15ull; b0 < end; b0 += 1024) {
      u64 a;
      u32 mnl, mgt;
      ss_nl_gt_masks(data, n, b0, lane, pos, end, a, mnl, mgt);
      c += (u32)__builtin_popcount(ss_fa_bnd(mnl, mgt, a, b0, lane, cnl, cgt));
    }
    u64 t = c;
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) cnt[i] = t;
  }
}

// rows[2 r] = sequence r's start, rows[2 r + 1] = its boundary B_k (the read's end); ord[r] = its ordinal
// within its section, rsec[r] = its section (relative to the batch).  Like k_ss_emit, an end goes to
// slot q and the next start to slot q + 1.
__global__ __launch_bounds__(256) void k_ss_fa_emit(const uint8_t *data, u64 n, const i64 *secs, u64 S, const u64 *cnt,
                                                    const u64 *base, u64 *rows, u32 *ord, u32 *rsec) {
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 i = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < S; i += nw) {
    const u64 nb = cnt[i], r0 = base[i];
    if (!nb) continue;
    const u64 pos = (u64)secs[2 * i], end = pos + (u64)secs[2 * i + 1];
    if (lane == 0) rows[2 * r0] = pos;
    u64 cnl = 0, cgt = 0, rank0 = 0;  // boundaries before this step
    for (u64 b0 = pos & ~15ull; b0 < end && rank0 < nb; b0 += 1024) {
      u64 a;
      u32 mnl, mgt;
      ss_nl_gt_masks(data, n, b0, lane, pos, end, a, mnl, mgt);
      u32 m = ss_fa_bnd(mnl, mgt, a, b0, lane, cnl, cgt);
      const u32 c = (u32)__builtin_popcount(m);
      const u32 incl = wave_scan_add(c);
      u64 q = rank0 + incl - c;
      for (; m && q < nb; m &= m - 1, ++q) {
        const u64 b = a + (u64)__builtin_ctz(m);
        rows[2 * (r0 + q) + 1] = b;
        ord[r0 + q] = (u32)q;
        rsec[r0 + q] = (u32)i;
        if (q + 1 < nb) rows[2 * (r0 + q + 1)] = b;
      }
      rank0 += (u32)__shfl((int)incl, 63, 64);
    }
  }
}

// rows[2 r] = line r's offset, rows[2 r + 1] = its length with the '\n' (the rows of the line index);
// rsec[r] = its section (relative to the batch).  cnt: the sections' '\n' counts.
__global__ __launch_bounds__(256) void k_ss_sam_emit(const uint8_t *data, u64 n, const i64 *secs, u64 S, const u64 *cnt,
                                                     const u64 *base, u64 *rows, u32 *rsec) {
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 i = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < S; i += nw) {
    const u64 nl = cnt[i], r0 = base[i];
    if (!nl) continue;
    const u64 pos = (u64)secs[2 * i], end = pos + (u64)secs[2 * i + 1];
    u64 start = pos, rank0 = 0;  // where the line open at the step's start begins; '\n' before this step
    for (u64 b0 = pos & ~15ull; b0 < end && rank0 < nl; b0 += 1024) {
      u64 a;
      u32 m = ss_nl_mask(data, n, b0, lane, pos, end, a);
      const u32 mnl = m;
      u32 tnl;
      const u32 pnl = ss_excl_max(ss_last_in_step(mnl, lane), lane, tnl);
      const u64 lstart = pnl ? b0 + pnl : start;  // the line open at the lane's first byte
      const u32 c = (u32)__builtin_popcount(m);
      const u32 incl = wave_scan_add(c);
      u64 q = rank0 + incl - c;
      for (; m && q < nl; m &= m - 1, ++q) {
        const u32 k = (u32)__builtin_ctz(m), below = (1u << k) - 1u;
        const u64 s = (mnl & below) ? a + 32 - (u64)__builtin_clz(mnl & below) : lstart;
        rows[2 * (r0 + q)] = s;
        rows[2 * (r0 + q) + 1] = a + k + 1 - s;
        rsec[r0 + q] = (u32)i;
      }
      if (tnl) start = b0 + tnl;
      rank0 += (u32)__shfl((int)incl, 63, 64);
    }
  }
}

// After the spans kernel of a FASTA or SAM batch: ctl[SS_BAD] is the first failing flat item (~0: none).
// ctl[SS_KE] = the items before it, ctl[SS_KEY] = its section within the batch (~0: none) and, count_nz
// (SAM: blank and '@' lines deliver nothing), ctl[SS_NDELIV] += the items before it with an output
// (zeroed by the caller).
__global__ __launch_bounds__(256) void k_ss_flat_finish(const u32 *rsec, const u64 *outlen, u64 K, int count_nz, u64 *ctl) {
  const u64 bad = ctl[SS_BAD];
  const u64 Ke = bad < K ? bad : K;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl[SS_KE] = Ke;
    ctl[SS_KEY] = bad < K ? (u64)rsec[bad] : ~0ull;
  }
  if (!count_nz) return;
  u32 c = 0;
  for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < Ke; k += (u64)gridDim.x * blockDim.x) c += outlen[k] != 0;
  u64 t = c;
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  if ((threadIdx.x & 63) == 0 && t) atomicAdd((unsigned long long *)&ctl[SS_NDELIV], (unsigned long long)t);
}

}  // namespace sidx

using namespace sidx;

static u32 ss_wave_grid(u64 S) { return (u32)((S + 3) / 4 < 262144 ? (S + 3) / 4 : 262144); }

// small_*: the small-section limit of each format; others / cuts: nsecs words each; ctl zeroed
extern "C" hipError_t sidx_stream_classify(const void *d_secs, u64 nsecs, u64 n, const int *fmt, u64 small_fastq,
                                           u64 small_fasta, u64 small_sam, u64 *ctl, u64 *others, u64 *cuts,
                                           hipStream_t s) {
  if (nsecs) hipLaunchKernelGGL(k_ss_classify, dim3((u32)((nsecs + 255) / 256)), dim3(256), 0, s, (const i64 *)d_secs,
                                nsecs, n, fmt, SmallLimits{small_fastq, small_fasta, small_sam}, ctl, others, cuts);
  return hipGetLastError();
}

extern "C" hipError_t sidx_stream_count(const uint8_t *data, u64 n, const void *d_secs, u64 S, u64 *cnt, hipStream_t s) {
  if (S) hipLaunchKernelGGL(k_ss_count, dim3(ss_wave_grid(S)), dim3(256), 0, s, data, n, (const i64 *)d_secs, S, cnt, 2u);
  return hipGetLastError();
}

// FASTA: cnt[i] = section i's boundaries (the sequences Read delivers before the one that ends at the
// section end)
extern "C" hipError_t sidx_stream_fa_count(const uint8_t *data, u64 n, const void *d_secs, u64 S, u64 *cnt,
                                           hipStream_t s) {
  if (S) hipLaunchKernelGGL(k_ss_fa_count, dim3(ss_wave_grid(S)), dim3(256), 0, s, data, n, (const i64 *)d_secs, S, cnt);
  return hipGetLastError();
}
// after the scan of cnt into base: rows (2 K words) / ord / rsec (K words) of the K sequences
extern "C" hipError_t sidx_stream_fa_emit(const uint8_t *data, u64 n, const void *d_secs, u64 S, const u64 *cnt,
                                          const u64 *base, u64 *rows, u32 *ord, u32 *rsec, hipStream_t s) {
  if (S) hipLaunchKernelGGL(k_ss_fa_emit, dim3(ss_wave_grid(S)), dim3(256), 0, s, data, n, (const i64 *)d_secs, S, cnt,
                            base, rows, ord, rsec);
  return hipGetLastError();
}
// SAM: cnt[i] = section i's '\n'-terminated lines; rows (2 K words) / rsec (K words) of the K lines
extern "C" hipError_t sidx_stream_sam_count(const uint8_t *data, u64 n, const void *d_secs, u64 S, u64 *cnt,
                                            hipStream_t s) {
  if (S) hipLaunchKernelGGL(k_ss_count, dim3(ss_wave_grid(S)), dim3(256), 0, s, data, n, (const i64 *)d_secs, S, cnt, 0u);
  return hipGetLastError();
}
extern "C" hipError_t sidx_stream_sam_emit(const uint8_t *data, u64 n, const void *d_secs, u64 S, const u64 *cnt,
                                           const u64 *base, u64 *rows, u32 *rsec, hipStream_t s) {
  if (S) hipLaunchKernelGGL(k_ss_sam_emit, dim3(ss_wave_grid(S)), dim3(256), 0, s, data, n, (const i64 *)d_secs, S, cnt,
                            base, rows, rsec);
  return hipGetLastError();
}
// after the spans of the K flat items (first failure in ctl[SS_BAD]): ctl[SS_KE], ctl[SS_KEY] and, count_nz,
// ctl[SS_NDELIV] (zeroed by the caller)
extern "C" hipError_t sidx_stream_flat_finish(const u32 *rsec, const u64 *outlen, u64 K, int count_nz, u64 *ctl,
                                              hipStream_t s) {
  const u64 nb = (K + 255) / 256;
  hipLaunchKernelGGL(k_ss_flat_finish, dim3((u32)(nb < 1 ? 1 : nb < 4096 ? nb : 4096)), dim3(256), 0, s, rsec, outlen, K,
                     count_nz, ctl);
  return hipGetLastError();
}

// after the scan of cnt into base: rows / ord / rsec of the K records, then ctl[SS_KEY] and ctl[SS_KE]
extern "C" hipError_t sidx_stream_index(const uint8_t *data, u64 n, const void *d_secs, u64 S, const u64 *cnt,
                                        const u64 *base, u64 K, u64 *rows, u32 *ord, u32 *rsec, u64 *ctl, hipStream_t s) {
  if (!S) return hipSuccess;
  const i64 *secs = (const i64 *)d_secs;
  hipLaunchKernelGGL(k_ss_emit, dim3(ss_wave_grid(S)), dim3(256), 0, s, data, n, secs, S, cnt, base, rows, ord, rsec, ctl);
  if (K) hipLaunchKernelGGL(k_ss_check, dim3((u32)((K + 255) / 256)), dim3(256), 0, s, data, n, secs, rows, ord, rsec, K,
                            ctl);
  hipLaunchKernelGGL(k_ss_finish, dim3(1), dim3(64), 0, s, base, K, ctl);
  return hipGetLastError();
}
