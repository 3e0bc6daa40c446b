// sidx_control.hip -- the control kernels of the MI355X record indexer: small kernels beside an
// index build's hot path (sidx_kernels.hip), each launched once per build or per slab exchange.
//
//   k_detect        format detection (multi.go:43-62), one workgroup, <= 32 KiB inspected
//   k_slab_guess    multi-GPU slabs: a slab's incoming state guessed from its first bytes
//   k_slab_combine  ... and the fold of the gathered slab summaries into this rank's plan
//   k_verify_rows   SHOCKIDX_VERIFY: the contiguity of a whole row table
#include <hip/hip_runtime.h>
#include <string.h>

#include "sidx_common.hpp"
#include "sidx_device.hpp"
#include "sidx_launch.hpp"

namespace sidx {

// ====================================================================================
// Multi-GPU slabs: guess a slab's incoming state, fold the gathered summaries
// ====================================================================================
// FASTQ: the first line of the slab that looks like a record start ('@' line, '+' two
// lines later, sequence and quality lines of equal length) fixes the line phase.
// FASTA: '\n' vs '>' closest before the slab start (armed bit).  SAM: class of the line
// open at the slab start.  LINE: nothing to guess.  One wave; verified after the exchange.
__global__ void k_slab_guess(const uint8_t *data, u64 n, u64 front, int fmt, u64 *out) {
  __shared__ u32 nlp[256];
  __shared__ u32 cnt;
  const int lane = threadIdx.x;
  u64 guess = 0;
  if (fmt == F_FASTQ) {
    const u64 lim = n < 4096 ? n : 4096;
    if (lane == 0) cnt = 0;
    __syncthreads();
    for (u64 b = 0; b < lim; b += 1024) {  // '\n' positions of the first 4 KiB, in order
      const u64 a = b + (u64)lane * 16;
      u32 m = 0;
      if (a < lim) m = eq16((a + 16 <= lim) ? load16(data + a) : load16_partial(data, a, lim), '\n');
      const u32 c = __popc(m);
      const u32 pre = wave_scan_add(c);
      const u32 base = cnt;
      u32 o = base + pre - c;
      while (m) { if (o < 256) nlp[o] = (u32)(a + __builtin_ctz(m)); ++o; m &= m - 1; }
      __syncthreads();
      if (lane == 63) cnt = base + pre;
      __syncthreads();
    }
    const u32 N = cnt < 256 ? cnt : 256;
    // candidate i: record starts after '\n' #i (local rank i): lines (i,i+1],(i+1,i+2]...
    bool ok = false;
    for (u32 i0 = 0; i0 + 4 < N; i0 += 64) {
      const u32 i = i0 + lane;
      ok = false;
      if (i + 4 < N) {
        const u32 s = nlp[i] + 1, e0 = nlp[i + 1], e1 = nlp[i + 2], e2 = nlp[i + 3], e3 = nlp[i + 4];
        ok = data[s] == '@' && e0 > s + 1 && data[e1 + 1] == '+' && (e1 - e0) == (e3 - e2) && e1 > e0 + 1;
      }
      const u64 bal = __ballot(ok);
      if (bal) { const u32 L = ctz64(bal); guess = (3u - ((i0 + L) & 3)) & 3; break; }
    }
  } else if (fmt == F_FASTA || fmt == F_SAM) {
    // closest '\n' / '>' before data[0] within `front` bytes (scan backwards 1 KiB per step)
    const u64 lim = front < 65536 ? front : 65536;
    i64 best = -1;
    u32 bestc = 0;
    for (u64 b = 0; b < lim && best < 0; b += 1024) {
      // window [-(b+1024), -b): lane k holds bytes [-(b+16k+16), -(b+16k))
      const u64 hi = b + (u64)lane * 16;  // distance of this chunk's end before data[0]
      u32 nlm = 0, gtm = 0;
      if (hi < lim) {
        const u64 take = (lim - hi) < 16 ? (lim - hi) : 16;
        const uint8_t *q = data - hi - take;
        const uint4 v = load16_partial(q, 0, take);
        nlm = eq16(v, '\n');
        gtm = fmt == F_FASTA ? eq16(v, '>') : 0u;  // bit j <-> the byte hi + take - j before data[0]
      }
      const u32 m = nlm | gtm;
      const u64 bal = __ballot(m != 0);
      if (bal) {
        const int L = (int)ctz64(bal);  // nearest chunk first
        const u32 mm = __shfl(m, L, 64);
        const u32 g = __shfl(gtm, L, 64);
        const u64 hiL = b + (u64)L * 16;
        const u64 takeL = (lim - hiL) < 16 ? (lim - hiL) : 16;
        const u32 j = 31 - __builtin_clz(mm);
        best = (i64)(hiL + takeL - j);
        bestc = (g >> j) & 1;  // 1: the nearest is '>'
      }
    }
    if (fmt == F_FASTA) {
      guess = (best < 0) ? 1 : (bestc ? 0 : 1);  // state = count 0 << 1 | armed
    } else {
      // SAM: byte before data[0] is '\n' -> FRESH; else class of the byte after the nearest '\n'
      if (front == 0 || best == 1) guess = 0;
      else if (best < 0) guess = 1;
      else guess = (data[-(best - 1)] == '@') ? 2 : 1;
    }
  }
  if (lane == 0) *out = guess;
}

template <int F>
__device__ __forceinline__ bool slab_compatible(u64 truth, u64 guess) {
  if (F == F_FASTQ) return (truth & 3) == (guess & 3);
  if (F == F_FASTA) return (truth & 1) == (guess & 1);
  if (F == F_SAM) return (truth & 3) == (guess & 3);
  return true;
}
template <int F>
__device__ __forceinline__ u64 slab_delta(u64 truth, u64 guess) {  // global - local record numbers
  if (F == F_FASTQ) return (truth - (guess & 3)) >> 2;
  if (F == F_FASTA) return (truth >> 1) - (guess >> 1);
  if (F == F_SAM) return (truth >> 2) - (guess >> 2);
  return truth - guess;
}

// The caller's expected build tag of every slab's summary (shockidx_slab_combine's expect_seq).
struct SeqExpect {
  u32 v[32];
  u32 on;
};
template <int F, class M>
__device__ void slab_combine(const SlabSummary *all, int world, int rank, const SeqExpect &ex, SlabPlan *out) {
  SlabPlan pl;
  pl.inconsistent = 0; pl.flags = 0; pl.err_rank = -1; pl.err_pos = 0; pl.err_len = 0; pl.code = ST_OK;
  pl.count = 0; pl.state_in = 0; pl.first_record = 0;
  u64 s = 0;  // state before slab 0 (file start)
  bool done = false;
  for (int q = 0; q < world; ++q) {
    const SlabSummary &x = all[q];
    if (ex.on && x.seq != ex.v[q]) pl.flags |= 32;  // a stale summary: never folded into a result
    const bool ok = slab_compatible<F>(s, x.state_in);
    if (!ok) pl.inconsistent |= 1u << q;
    const u64 delta = slab_delta<F>(s, x.state_in);
    if (q == rank) { pl.state_in = s; pl.first_record = delta + x.row_base; }
    pl.flags |= x.flags & ~RF_CAPACITY;
    if (!done && ok) {
      if (x.key != KEY_NONE) {
        pl.count = (x.key >> KEY_REC_SHIFT) + delta;
        pl.code = (u32)(x.key & 15);
        if (pl.code == ST_FA_INVALID) { pl.err_rank = q; pl.err_pos = x.err_pos; pl.err_len = x.err_len; }
        done = true;
      } else if (q == world - 1) {
        pl.count = x.natural + delta;
      }
    }
    s = M::apply(s, x.agg);
  }
  *out = pl;
}

__global__ void k_slab_combine(const SlabSummary *all, int world, int rank, int fmt, const SeqExpect ex, SlabPlan *out) {
  if (threadIdx.x || blockIdx.x) return;
  if (fmt == F_FASTQ) slab_combine<F_FASTQ, CountMonoid>(all, world, rank, ex, out);
  else if (fmt == F_FASTA) slab_combine<F_FASTA, FastaMonoid>(all, world, rank, ex, out);
  else if (fmt == F_SAM) slab_combine<F_SAM, SamMonoid>(all, world, rank, ex, out);
  else slab_combine<F_LINE, CountMonoid>(all, world, rank, ex, out);
}

// ====================================================================================
// k_detect: multi.go:43-62 over the zero-padded first 32768 bytes (fasta, fastq, sam)
// ====================================================================================
struct DetBuf {
  const uint8_t *d;  // the head, staged in LDS: m bytes, zeros from there to 32768 (not stored)
  u32 m;
  __device__ __forceinline__ u32 at(u64 i) const { return i < m ? (u32)d[i] : 0u; }
};
__device__ __forceinline__ bool dS(u32 c) { return !(c == '\t' || c == '\n' || c == '\f' || c == '\r' || c == ' '); }
__device__ __forceinline__ bool dSST(u32 c) { return !(c == '\n' || c == '\f' || c == '\r'); }
__device__ __forceinline__ bool dNR(u32 c) { return c == '\n' || c == '\r'; }
__device__ __forceinline__ bool dAlpha(u32 c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

// The matchers run wave-wide: every "class run" of the regex is skipped 64 bytes at a time
// (one byte per lane, a ballot for the first byte outside the class); single-byte checks are
// uniform LDS reads.  skip(b, i, P): the first j >= i with !P(b[j]), N if none.
template <class P>
__device__ __forceinline__ u64 det_skip(const DetBuf &b, u64 i, P pred) {
  const u64 N = 32768;
  const int lane = threadIdx.x & 63;
  u64 base = i;
  for (; base < N && base < b.m; base += 64) {
    const u64 q = base + (u64)lane;
    const u64 m = __ballot(q < N && !pred(b.at(q)));
    if (m) return base + (u64)__builtin_ctzll(m);
  }
  // only padding is left: every byte of it is zero
  return (base < N && !pred(0u)) ? base : N;
}
__device__ __forceinline__ bool dLetDash(u32 c) { return dAlpha(c) || c == '-'; }

// fasta.go:22  ^[\n\r]*>\S+[\S\t ]*[\n\r]+[A-Za-z\- ]+
__device__ bool det_fasta(const DetBuf &b) {
  const u64 N = 32768;
  u64 i = det_skip(b, 0, dNR);
  if (i >= N || b.at(i) != '>') return false;
  ++i;
  if (i >= N || !dS(b.at(i))) return false;
  i = det_skip(b, i + 1, dSST);
  if (i >= N || !dNR(b.at(i))) return false;
  i = det_skip(b, i, dNR);
  if (i >= N) return false;
  const u32 c = b.at(i);
  return dAlpha(c) || c == '-' || c == ' ';
}
// fastq.go:22  ^[\n\r]*@\S+[\S\t ]*[\n\r]+[A-Za-z\-]+[\n\r]+\+[\S\t ]*[\n\r]+\S*[\n\r]+
__device__ bool det_fastq(const DetBuf &b) {
  const u64 N = 32768;
  u64 i = det_skip(b, 0, dNR);
  if (i >= N || b.at(i) != '@') return false;
  ++i;
  if (i >= N || !dS(b.at(i))) return false;
  i = det_skip(b, i + 1, dSST);
  if (i >= N || !dNR(b.at(i))) return false;
  i = det_skip(b, i, dNR);
  if (i >= N || !dLetDash(b.at(i))) return false;
  i = det_skip(b, i, dLetDash);
  if (i >= N || !dNR(b.at(i))) return false;
  i = det_skip(b, i, dNR);
  if (i >= N || b.at(i) != '+') return false;
  i = det_skip(b, i + 1, dSST);
  const u64 k = det_skip(b, i, dNR) - i;
  if (k == 0) return false;
  if (k >= 2) return true;
  i = det_skip(b, i + 1, dS);
  return i < N && dNR(b.at(i));
}
// sam.go:17  ^[\n\r]*[@[A-Z][A-Z][ \t]+[\S \t]+[\n\r]]*
__device__ bool det_sam(const DetBuf &b) {
  const u64 N = 32768;
  u64 i = det_skip(b, 0, dNR);
  if (i >= N) return false;
  u32 c = b.at(i);
  if (!(c == '@' || c == '[' || (c >= 'A' && c <= 'Z'))) return false;
  ++i;
  c = b.at(i);
  if (i >= N || !(c >= 'A' && c <= 'Z')) return false;
  ++i;
  c = b.at(i);
  if (i >= N || !(c == ' ' || c == '\t')) return false;
  ++i;
  const u64 e = det_skip(b, i, dSST);
  return e > i && e < N && dNR(b.at(e));
}

// The three matchers over a staged head of m bytes, one per wave (side by side), each wave-wide;
// called by the whole workgroup (at least three waves).  out[0]: the format, out[1]: the match mask.
__device__ void det_match(const uint8_t *head, u32 m, int *out) {
  __shared__ int part[3];
  const DetBuf b{head, m};
  if (threadIdx.x < 192) {
    const int w = threadIdx.x >> 6;
    const int r = w == 0 ? (det_fasta(b) ? 1 : 0) : w == 1 ? (det_fastq(b) ? 2 : 0) : (det_sam(b) ? 4 : 0);
    if ((threadIdx.x & 63) == 0) part[w] = r;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int mk = part[0] | part[1] | part[2];
  out[0] = (mk & 1) ? F_FASTA : (mk & 2) ? F_FASTQ : (mk & 4) ? F_SAM : F_NONE;
  out[1] = mk;
}

// The head is staged into LDS by the whole workgroup (16 B per lane, every load in flight at
// once), then three waves run the three matchers against LDS.
constexpr int DET_THREADS = 512;
__global__ __launch_bounds__(DET_THREADS) void k_detect(const uint8_t *data, u64 n, int *out) {
  __shared__ __align__(16) uint8_t head[32768];
  const u64 m = n < 32768 ? n : 32768;
  constexpr int PER = 32768 / 16 / DET_THREADS;
  uint4 v[PER];  // every load in flight before the first LDS store
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const u64 a = (u64)(threadIdx.x + k * DET_THREADS) * 16;
    v[k] = make_uint4(0, 0, 0, 0);
    if (a + 16 <= m) v[k] = load16(data + a);
    else if (a < m) v[k] = load16_partial(data, a, m);
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) *reinterpret_cast<uint4 *>(&head[(u64)(threadIdx.x + k * DET_THREADS) * 16]) = v[k];
  __syncthreads();
  det_match(head, 32768u, out);
}

// One workgroup per section {int64 pos, int64 len} of data: DetermineFormat over the section's
// first min(len, 32768) bytes (multi.go:43-62 runs once per section reader).  pos is arbitrary, so
// the head is staged from 16-byte aligned loads, byte by byte into LDS; the padding is not stored
// (DetBuf::at).  out[s]: the format.  The caller has checked the sections against n.
constexpr int DETB_THREADS = 256;
__global__ __launch_bounds__(DETB_THREADS) void k_detect_sections(const uint8_t *data, u64 n, const i64 *secs,
                                                                  u64 nsecs, int *out) {
  __shared__ __align__(16) uint8_t head[32768];
  __shared__ int res[2];
  const u64 sidx = blockIdx.x;
  if (sidx >= nsecs) return;
  if (secs[2 * sidx] < 0 || secs[2 * sidx + 1] < 0 || (u64)secs[2 * sidx] > n ||
      (u64)secs[2 * sidx + 1] > n - (u64)secs[2 * sidx]) {  // outside the node: the caller's error, nothing read
    if (threadIdx.x == 0) out[sidx] = F_NONE;
    return;
  }
  const u64 pos = (u64)secs[2 * sidx], len = (u64)secs[2 * sidx + 1];
  const u32 m = (u32)(len < 32768 ? len : 32768);
  const u64 lo = pos & ~15ull, hi = pos + m;
  for (u64 a = lo + 16ull * threadIdx.x; a < hi; a += 16ull * DETB_THREADS) {
    const uint4 v = (a + 16 <= n) ? load16(data + a) : load16_partial(data, a, n);
    const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const u64 p = a + k;
      if (p >= pos && p < hi) head[p - pos] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
  }
  __syncthreads();
  det_match(head, m, res);
  if (threadIdx.x == 0) out[sidx] = res[0];
}

// Whole-table check (SHOCKIDX_VERIFY builds, on in the GPU test suite): every row starts where
// the previous one ends (record.go:51-83), over the rows the build reported (DevResult::count,
// read on the device after the pipeline); a violation sets the internal-error flag.
__global__ __launch_bounds__(256) void k_verify_rows(const u64 *rows, u64 row_base, u64 row_cap, DevResult *res) {
  const DevResult r = *res;
  if (r.flags & (RF_CAPACITY | RF_MISSPEC)) return;  // a capacity overflow or a failed speculation: re-run anyway
  const u64 nr = r.count > row_base ? r.count - row_base : 0;
  const u64 n = nr < row_cap ? nr : row_cap;
  bool bad = false;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i + 1 < n; i += (u64)gridDim.x * 256) {
    const ulonglong2 a = reinterpret_cast<const ulonglong2 *>(rows)[i];
    bad |= a.x + a.y != rows[2 * (i + 1)];
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&res->flags, RF_INTERNAL);
}
}  // namespace sidx

// ====================================================================================
// Host launch wrappers (declared in sidx_launch.hpp)
// ====================================================================================
using namespace sidx;

extern "C" hipError_t sidx_launch_detect(const uint8_t *d, u64 n, int *d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_detect, dim3(1), dim3(DET_THREADS), 0, s, d, n, d_out);
  return hipGetLastError();
}

extern "C" hipError_t sidx_launch_detect_sections(const uint8_t *d, u64 n, const void *d_secs, u64 nsecs, int *d_out,
                                                  hipStream_t s) {
  if (nsecs) hipLaunchKernelGGL(k_detect_sections, dim3((u32)nsecs), dim3(DETB_THREADS), 0, s, d, n, (const i64 *)d_secs,
                                nsecs, d_out);
  return hipGetLastError();
}

extern "C" hipError_t sidx_launch_slab_guess(const uint8_t *d, u64 n, u64 front, int fmt, u64 *d_out,
                                             hipStream_t s) {
  hipLaunchKernelGGL(k_slab_guess, dim3(1), dim3(64), 0, s, d, n, front, fmt, d_out);
  return hipGetLastError();
}

extern "C" hipError_t sidx_launch_slab_combine(const void *d_all, int world, int rank, int fmt, const uint32_t *expect,
                                               void *d_plan, hipStream_t s) {
  SeqExpect ex;
  memset(&ex, 0, sizeof ex);
  if (expect) {
    ex.on = 1;
    for (int q = 0; q < world && q < 32; ++q) ex.v[q] = expect[q];
  }
  hipLaunchKernelGGL(k_slab_combine, dim3(1), dim3(64), 0, s, (const SlabSummary *)d_all, world, rank, fmt, ex,
                     (SlabPlan *)d_plan);
  return hipGetLastError();
}

extern "C" hipError_t sidx_launch_verify_rows(const u64 *rows, u64 row_base, u64 row_cap, DevResult *d_res, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_rows, dim3(1024), dim3(256), 0, s, rows, row_base, row_cap, d_res);
  return hipGetLastError();
}
