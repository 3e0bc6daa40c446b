// sidx_plan.hip -- gfx950 kernels of the download plan (shockidx_download_plan): the section list
// of a whole ?download&index=X&part=a&part=b... request, built on the device in a number of
// launches that does not grow with the number of parts.
//
// Reference semantics (paths relative to shock-server/):
//   controller/node/single.go:372-483   the s.R = append(...) loops: the parts in order, each part's
//       Idx.Part section or Idx.Range records appended to one list; for a subset node's chunkrecord
//       index every record of the matrix index becomes "start-stop" and goes through a second
//       Idx.Range over the node's record index (:401-425)
//   node/file/index/index.go:67-193     Idx.Part / Idx.Range
//
// A segmented form of the k_range_* kernels (sidx_subset.hip): the row visits of all parts are
// laid end to end (the host scans the parts' visit counts), every visit finds its segment by
// binary search in the scanned offsets, a visit starts a section when it is its segment's first or
// its row does not continue the previous one (curLen == nextPos - curPos, index.go:162,170), the
// flag scan numbers the sections, and two passes write pos and len.  Sections never merge across
// segments: Go appends each Range's records as they are.  A row past the table reads as the last
// row of the segment's own walk (plan_row with the segment's a0), so nothing leaks between parts.
// Level 2 of CHUNK_RANGE runs the same passes with the level-1 records as segments.
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"
#include "sidx_launch.hpp"
#include "sidx_plan.hpp"
#include "sidx_plan_host.hpp"

namespace sidx {

// (as in sidx_subset.hip) row i of a walk that began at row a0
__device__ __forceinline__ ulonglong2 plan_row(const u64 *rows, u64 nrows, u64 a0, u64 i) {
  if (i < nrows) return reinterpret_cast<const ulonglong2 *>(rows)[i];
  if (a0 < nrows) return reinterpret_cast<const ulonglong2 *>(rows)[nrows - 1];
  return make_ulonglong2(0, 0);
}

// the segment of visit j: the last s < nseg with off[s] <= j (off ascending, off[0] = 0; an empty
// segment shares its offset with the next one and is never the last)
__device__ __forceinline__ u64 plan_seg(const u64 *off, u64 nseg, u64 j) {
  u64 lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const u64 mid = (lo + hi) >> 1;
    if (off[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void k_plan_init(u64 *ctl) {
  if (threadIdx.x < PC_NWORDS) ctl[threadIdx.x] = threadIdx.x == PC_ERRKEY ? ~0ull : 0;
}

// visit j = row a0[s] + (j - off[s]) of segment s; vseg[j] = s for the emit passes
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_flags(const u64 *rows, u64 nrows, const u64 *a0, const u64 *off,
                                                             u64 nseg, u64 V, u32 *flags, u32 *vseg) {
  const u64 j = (u64)blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (j >= V) return;
  const u64 s = plan_seg(off, nseg, j), k = j - off[s], a = a0[s];
  u32 f = 1;
  if (k > 0) {
    const ulonglong2 c = plan_row(rows, nrows, a, a + k), p = plan_row(rows, nrows, a, a + k - 1);
    f = c.x != p.x + p.y;
  }
  flags[j] = f;
  vseg[j] = (u32)s;
}

// the total of a flag scan into a control word
__global__ void k_plan_total(const u32 *flags, const u64 *id, u64 V, u64 *ctl, int word) {
  ctl[word] = id[V - 1] + flags[V - 1];
}

// Sections are written only when all of them fit (ctl[word] <= cap): a short capacity writes nothing.
// part (optional): the part each section belongs to -- segpart[s], or s itself at level 1.
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_pos(const u64 *rows, u64 nrows, const u64 *a0, const u64 *off,
                                                           const u32 *vseg, u64 V, const u32 *flags, const u64 *id,
                                                           const u64 *ctl, int word, u64 cap, u64 *out, u32 *part,
                                                           const u32 *segpart) {
  const u64 j = (u64)blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (j >= V || ctl[word] > cap || !flags[j]) return;
  const u32 s = vseg[j];
  const u64 a = a0[s];
  out[2 * id[j]] = plan_row(rows, nrows, a, a + (j - off[s])).x;
  if (part) part[id[j]] = segpart ? segpart[s] : s;
}
// the last visit of every section: curLen, the section's lengths summed (mod 2^64) = the end of its
// last row minus its pos; size (optional): the lengths of all sections, one atomic per workgroup
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_len(const u64 *rows, u64 nrows, const u64 *a0, const u64 *off,
                                                           const u32 *vseg, u64 V, const u32 *flags, const u64 *id,
                                                           const u64 *ctl, int word, u64 cap, u64 *out, u64 *size) {
  __shared__ u64 wsum[PLAN_THREADS / 64];
  const u64 j = (u64)blockIdx.x * PLAN_THREADS + threadIdx.x;
  u64 len = 0;
  if (j < V && ctl[word] <= cap && (j + 1 == V || flags[j + 1])) {
    const u32 s = vseg[j];
    const u64 a = a0[s];
    const ulonglong2 c = plan_row(rows, nrows, a, a + (j - off[s]));
    const u64 r = id[j] + flags[j] - 1;
    len = c.x + c.y - out[2 * r];
    out[2 * r + 1] = len;
  }
  if (!size) return;
  for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = len;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (u32 w = 0; w < PLAN_THREADS / 64; ++w) t += wsum[w];
    if (t) atomicAdd((unsigned long long *)size, (unsigned long long)t);
  }
}

// Level 2 of CHUNK_RANGE (single.go:411-414): every level-1 record (c0, c1) as the record range
// "start-stop" (chunk_segment, sidx_plan_host.hpp); an invalid one reports its place in Go's order.
// The grid covers V1, a bound of the record count; the slots past the count are empty segments.
// A segment longer than one plan may visit counts as one visit more than that (the total then
// says so, and the scan's sums stay below 2^62).
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_segs(const u64 *recs, const u32 *part, u64 bound, u64 *ctl,
                                                            i64 rec_length, u64 *a0, u64 *nr) {
  const u64 s = (u64)blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (s >= bound) return;
  sidx_plan::u64 a = 0, n = 0;
  if (s < ctl[PC_N1]) {
    if (!sidx_plan::chunk_segment((i64)recs[2 * s], (i64)recs[2 * s + 1], rec_length, &a, &n))
      atomicMin((unsigned long long *)&ctl[PC_ERRKEY], (unsigned long long)(((u64)part[s] << 32) | s));
    if (n > sidx_plan::MAX_VISITS) n = sidx_plan::MAX_VISITS + 1;
  }
  a0[s] = a;
  nr[s] = n;
}
__global__ void k_plan_total64(const u64 *nr, const u64 *off, u64 n, u64 *ctl, int word) {
  ctl[word] = off[n - 1] + nr[n - 1];
}

// Idx.Part per part (index.go:86-99, :107-114): rows a0 and b0 (the same row for "N"), a row past
// the table as zeros; (pos, length) = (s.pos, e.pos - s.pos + e.len), which is the row itself when
// a0 == b0
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_part(const u64 *rows, u64 nrows, const u64 *a0, const u64 *b0,
                                                            u64 P, u64 *out, u64 *size) {
  __shared__ u64 wsum[PLAN_THREADS / 64];
  const u64 p = (u64)blockIdx.x * PLAN_THREADS + threadIdx.x;
  u64 len = 0;
  if (p < P) {
    const u64 a = a0[p], b = b0[p];
    const ulonglong2 z = make_ulonglong2(0, 0);
    const ulonglong2 sr = a < nrows ? reinterpret_cast<const ulonglong2 *>(rows)[a] : z;
    const ulonglong2 er = b < nrows ? reinterpret_cast<const ulonglong2 *>(rows)[b] : z;
    len = er.x - sr.x + er.y;
    out[2 * p] = sr.x;
    out[2 * p + 1] = len;
  }
  for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = len;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (u32 w = 0; w < PLAN_THREADS / 64; ++w) t += wsum[w];
    if (t) atomicAdd((unsigned long long *)size, (unsigned long long)t);
  }
}

}  // namespace sidx

using namespace sidx;

namespace {
inline u32 nblk(u64 n) { return (u32)((n + PLAN_THREADS - 1) / PLAN_THREADS); }
}

extern "C" hipError_t sidx_plan_init(u64 *ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_init, dim3(1), dim3(64), 0, s, ctl);
  return hipGetLastError();
}

// One level of a plan over V > 0 visits of nseg segments (a0, off: device arrays, off the exclusive
// scan of the segments' visit counts): the section count into ctl[word], then the sections into out
// when they fit cap.  flags, vseg: V words each; id: V; tmp: the flag scan's workspace.
extern "C" hipError_t sidx_plan_level(const u64 *rows, u64 nrows, const u64 *a0, const u64 *off, u64 nseg, u64 V,
                                      u32 *flags, u32 *vseg, u64 *id, void *tmp, size_t *tmp_bytes, u64 *ctl, int word,
                                      u64 cap, u64 *out, u32 *part, const u32 *segpart, u64 *size, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_flags, dim3(nblk(V)), dim3(PLAN_THREADS), 0, s, rows, nrows, a0, off, nseg, V, flags, vseg);
  hipError_t e = sidx_scan_flags(flags, id, V, tmp, tmp_bytes, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_plan_total, dim3(1), dim3(1), 0, s, flags, id, V, ctl, word);
  hipLaunchKernelGGL(k_plan_pos, dim3(nblk(V)), dim3(PLAN_THREADS), 0, s, rows, nrows, a0, off, vseg, V, flags, id, ctl,
                     word, cap, out, part, segpart);
  hipLaunchKernelGGL(k_plan_len, dim3(nblk(V)), dim3(PLAN_THREADS), 0, s, rows, nrows, a0, off, vseg, V, flags, id, ctl,
                     word, cap, out, size);
  return hipGetLastError();
}

// The level-2 segments of `bound` >= 1 level-1 record slots: a0, nr, their scan off, and the visit
// total into ctl[PC_V2]
extern "C" hipError_t sidx_plan_segments(const u64 *recs, const u32 *part, u64 bound, u64 *ctl, i64 rec_length, u64 *a0,
                                         u64 *nr, u64 *off, void *tmp, size_t *tmp_bytes, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_segs, dim3(nblk(bound)), dim3(PLAN_THREADS), 0, s, recs, part, bound, ctl, rec_length, a0, nr);
  hipError_t e = sidx_scan_u64(nr, off, bound, tmp, tmp_bytes, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_plan_total64, dim3(1), dim3(1), 0, s, nr, off, bound, ctl, (int)PC_V2);
  return hipGetLastError();
}

extern "C" hipError_t sidx_plan_part(const u64 *rows, u64 nrows, const u64 *a0, const u64 *b0, u64 P, u64 *out,
                                     u64 *size, hipStream_t s) {
  if (P) hipLaunchKernelGGL(k_plan_part, dim3(nblk(P)), dim3(PLAN_THREADS), 0, s, rows, nrows, a0, b0, P, out, size);
  return hipGetLastError();
}
