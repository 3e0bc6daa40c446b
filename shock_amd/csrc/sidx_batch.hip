// sidx_batch.hip -- gfx950 kernels of the batch build: the index of many small nodes
// {int64 pos, int64 len} of one arena in HBM in one call.  Node i's result is that of the single
// build (sidx_kernels.hip) over the bytes [pos, pos + len) alone: the same validators
// (sidx_validate.hpp) run over accessors that end at the node's end with eof = 1 and front = 0,
// on positions relative to the node's first byte, so nothing outside the node is read as part of it.
//
//   k_b_classify  one lane per node: the range check; the nodes longer than the small limit
//                 (left to the single build) are reported; the first-terminator slots reset
//   (k_detect_sections, sidx_control.hip: DetermineFormat per node when no format is given)
//   k_b_count     one wave per node: its format's monoid folded over the node, step by step, and
//                 from the final state the rows it has when no record ends it early
//   (exclusive scan over the nodes, sidx_scan.hpp: each node's first row)
//   k_b_layout    the table's extent; rows may be written only if the list is valid and it fits
//   k_b_emit      one wave per node: the start of every candidate record into the node's region
//   k_b_check     one lane per record: the format's validator; the row's length, or the node's
//                 first terminating (record, status) by a 64-bit atomicMin; a record the lane
//                 would have to scan far for is marked for
//   k_b_fix       one wave per marked record: the same validator over the wave accessor
//   k_b_finish    one lane per node: slot + natural count -> count, status, terminating code and
//                 the FASTA piece; with verify, the finished table's invariants
//
// A wave per node, 16 bytes per lane and step, no LDS; nodes do not share a wave (the reason is
// in sidx_stream.hip's header: wave slots, not lanes, hide the one round of loads a node takes).
// Every kernel dispatches on the node's own format word, so the launches of a call do not depend on
// how many nodes there are, which formats occur or how they interleave.
#include <hip/hip_runtime.h>

#include "../../include/shockidx.h"
#include "sidx_batch.hpp"
#include "sidx_batch_host.hpp"
#include "sidx_common.hpp"
#include "sidx_device.hpp"
#include "sidx_launch.hpp"
#include "sidx_seg.hpp"
#include "sidx_validate.hpp"

namespace sidx {

constexpr u64 B_DEFER = ~0ull;     // a row's length word: the record waits for k_b_fix
constexpr u64 B_LANE_SCAN = 512;   // bytes a lane searches before it leaves the record to a wave

struct BNode {
  const uint8_t *g;  // the node's first byte (16-byte aligned)
  u64 len;
  int fmt;
  bool batched;      // the walk takes it (small, and of a format)
};
__device__ __forceinline__ BNode b_node(const BatchArgs &p, u64 i) {
  BNode nd;
  nd.g = p.data + (u64)p.nodes[2 * i];
  nd.len = (u64)p.nodes[2 * i + 1];
  nd.fmt = p.nfmt[i];
  nd.batched = batch_is_small(nd.len, p.small) && nd.fmt != F_NONE;
  return nd;
}

// the 16 bytes of the lane at a (relative to the node), clipped at the node's end: zeros beyond
__device__ __forceinline__ uint4 b_load(const BNode &nd, u64 a) {
  return (a + 16 <= nd.len) ? load16(nd.g + a) : load16_partial(nd.g, a, nd.len);
}
// the lane's bytes of the step at b0, their '\n' and class-X masks and how many lie in the node
__device__ __forceinline__ u32 b_masks(const BNode &nd, u64 b0, int lane, u32 xc, u64 &a, u32 &mnl, u32 &mx) {
  a = b0 + 16ull * lane;
  mnl = mx = 0;
  if (a >= nd.len) return 0;
  const uint4 v = b_load(nd, a);
  const u32 k = nd.len - a < 16 ? (u32)(nd.len - a) : 16u;
  const u32 keep = (1u << k) - 1u;
  mnl = eq16(v, '\n') & keep;
  if (xc) mx = eq16(v, xc) & keep;
  return k;
}

__global__ __launch_bounds__(256) void k_b_classify(const BatchArgs p) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.K) return;
  const i64 pos = p.nodes[2 * i], len = p.nodes[2 * i + 1];
  p.key[i] = ~0ull;
  if (p.fmt != F_NONE) p.nfmt[i] = p.fmt;
  if (!batch_node_ok(pos, len, p.data_len)) {
    atomicOr((unsigned long long *)&p.ctl[BC_INVALID], 1ull);
    return;
  }
  if (!batch_is_small((u64)len, p.small)) {
    const u64 k = atomicAdd((unsigned long long *)&p.ctl[BC_NSINGLE], 1ull);
    p.singles[k] = BatchSingle{i, pos, len};  // at most K entries
  }
}

// the node's final monoid state: the lanes' 16-byte segments folded in byte order, step after step
template <class M>
__device__ __forceinline__ u64 b_fold(const BNode &nd, u32 xc, int lane) {
  u64 state = 0;
  for (u64 b0 = 0; b0 < nd.len; b0 += BATCH_STEP) {
    u64 a;
    u32 mnl, mx;
    const u32 k = b_masks(nd, b0, lane, xc, a, mnl, mx);
    state = M::apply(state, wave_total_in_order<M>(M::seg(mnl, mx, k), lane));
  }
  return state;
}

__global__ __launch_bounds__(256) void k_b_count(const BatchArgs p) {
  if (p.ctl[BC_INVALID]) return;
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 i = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < p.K; i += nw) {
    const BNode nd = b_node(p, i);
    u64 nat = 0;
    if (nd.fmt == F_FASTA) nat = natural_count(F_FASTA, b_fold<FastaMonoid>(nd, '>', lane));
    else if (nd.fmt == F_SAM) nat = natural_count(F_SAM, b_fold<SamMonoid>(nd, '@', lane));
    else if (nd.fmt == F_FASTQ || nd.fmt == F_LINE) nat = natural_count(nd.fmt, b_fold<CountMonoid>(nd, 0, lane));
    if (lane == 0) p.nat[i] = nat;
  }
}

__global__ void k_b_layout(const BatchArgs p) {
  if (threadIdx.x || blockIdx.x) return;
  const u64 total = p.ctl[BC_INVALID] ? 0 : p.base[p.K - 1] + p.nat[p.K - 1];
  p.ctl[BC_TOTAL] = total;
  p.ctl[BC_GO] = !p.ctl[BC_INVALID] && total <= p.row_cap;
}

// candidate k (1 .. nat - 1) of the node whose region starts at row r0 begins at s; one past the
// natural count is a disagreement between the fold and the walk
__device__ __forceinline__ void b_put(const BatchArgs &p, u64 r0, u64 nat, u64 k, u64 s) {
  if (k < nat) p.rows[2 * (r0 + k)] = s;
  else atomicOr((unsigned long long *)&p.ctl[BC_INTERNAL], 1ull);
}

// The starts of the node's candidate records, in order, into rows[2 (r0 + k)]; returns how many
// candidates after record 0 the walk met (every lane).
//   FASTQ: the byte after every '\n' of rank 3 mod 4      line: the byte after every '\n'
//   SAM:   the byte after a terminator line's '\n' (a line of at least one byte that does not
//          start with '@', sam.go:83-98)
//   FASTA: every '>' with a '\n' since the previous '>' of the node (the FastaMonoid's rule from
//          state 0: the node's first '>' is a boundary iff a '\n' precedes it)
template <int F>
__device__ __forceinline__ u64 b_emit_node(const BatchArgs &p, const BNode &nd, u64 r0, u64 nat, int lane) {
  constexpr u32 xc = F == F_FASTA ? (u32)'>' : 0u;
  u64 rank0 = 0;              // FASTQ / line: '\n' before this step; FASTA / SAM: candidates before it
  u64 cnl = 0, cgt = 0;       // FASTA: the last '\n' / '>' before this step (position + 1, 0: none)
  u64 start = 0;              // SAM: where the line open at the step's first byte begins
  for (u64 b0 = 0; b0 < nd.len; b0 += BATCH_STEP) {
    u64 a;
    u32 mnl, mx;
    b_masks(nd, b0, lane, xc, a, mnl, mx);
    u32 m = mnl;  // the candidates' bits
    if (F == F_FASTA) m = ss_fa_bnd(mnl, mx, a, b0, lane, cnl, cgt);
    if (F == F_SAM) {
      u32 tnl;
      const u32 pnl = ss_excl_max(ss_last_in_step(mnl, lane), lane, tnl);
      const u64 lstart = pnl ? b0 + pnl : start;  // the line open at the lane's first byte
      m = 0;
      for (u32 w = mnl; w; w &= w - 1) {
        const u32 k = (u32)__builtin_ctz(w), below = (1u << k) - 1u;
        const u64 s = (mnl & below) ? a + 32 - (u64)__builtin_clz(mnl & below) : lstart;
        if (s < a + k && nd.g[s] != '@') m |= 1u << k;
      }
      if (tnl) start = b0 + tnl;
    }
    const u32 c = (u32)__builtin_popcount(m);
    const u32 incl = wave_scan_add(c);
    u64 q = rank0 + incl - c;
    for (; m; m &= m - 1, ++q) {
      const u64 at = a + (u64)__builtin_ctz(m);
      if (F == F_FASTQ) {
        if ((q & 3) == 3) b_put(p, r0, nat, (q + 1) >> 2, at + 1);
      } else if (F == F_FASTA) {
        b_put(p, r0, nat, q + 1, at);
      } else {
        b_put(p, r0, nat, q + 1, at + 1);
      }
    }
    rank0 += (u32)__shfl((int)incl, 63, 64);
  }
  return F == F_FASTQ ? rank0 >> 2 : rank0;
}

__global__ __launch_bounds__(256) void k_b_emit(const BatchArgs p) {
  if (!p.ctl[BC_GO]) return;
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 i = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < p.K; i += nw) {
    const BNode nd = b_node(p, i);
    if (!nd.batched) continue;
    const u64 r0 = p.base[i], nat = p.nat[i];
    if (lane == 0) p.rows[2 * r0] = 0;  // record 0 (nat >= 1 for every format)
    u64 met;
    if (nd.fmt == F_FASTQ) met = b_emit_node<F_FASTQ>(p, nd, r0, nat, lane);
    else if (nd.fmt == F_FASTA) met = b_emit_node<F_FASTA>(p, nd, r0, nat, lane);
    else if (nd.fmt == F_SAM) met = b_emit_node<F_SAM>(p, nd, r0, nat, lane);
    else met = b_emit_node<F_LINE>(p, nd, r0, nat, lane);
    if (lane == 0 && met + 1 != nat) atomicOr((unsigned long long *)&p.ctl[BC_INTERNAL], 1ull);
  }
}

// Lane accessor over one node in global memory, positions relative to the node.  A search that does
// not end within B_LANE_SCAN bytes returns FR_DEFER: the record goes to k_b_fix's wave accessor.
struct NodeAcc {
  const uint8_t *g;
  u64 end;
  int eof;
  u64 front;
  __device__ __forceinline__ u32 byte(u64 q) const { return g[q]; }
  __device__ __forceinline__ const uint8_t *ptr() const { return g; }
  __device__ __forceinline__ u64 base() const { return 0; }
  __device__ u32 find(int cls, u64 q, u64 lim, u64 &out) const {
    const u64 hi = lim < end ? lim : end;
    const u64 stop = hi - q > B_LANE_SCAN && q < hi ? q + B_LANE_SCAN : hi;
    const u32 xc = cls == C_X ? (u32)'>' : (u32)'\n';
    for (; q < stop; ++q)
      if ((g[q] == xc) != (cls == C_NOTNL)) { out = q; return FR_FOUND; }
    return stop == hi ? FR_NONE : FR_DEFER;
  }
};

// the node whose region holds row r: the last one whose first row is at or before r (a node without
// rows shares its first row with the next one)
__device__ __forceinline__ u64 b_node_of_row(const u64 *base, u64 K, u64 r) {
  u64 lo = 0, hi = K;  // base[lo] <= r < base[hi]
  while (hi - lo > 1) {
    const u64 mid = lo + (hi - lo) / 2;
    if (base[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// record k of the node (its row r, its start already there) through its format's validator
template <class A>
__device__ __forceinline__ u32 b_validate(A &acc, int fmt, u64 k, u64 s, u64 &len, u64 &epos, u64 &elen) {
  if (fmt == F_FASTQ) return run_record<F_FASTQ>(acc, s, 0, len, epos, elen);
  if (fmt == F_FASTA) return run_record<F_FASTA>(acc, s, k ? s + 1 : 0, len, epos, elen);  // lo: past the '>' it starts with
  if (fmt == F_SAM) return run_record<F_SAM>(acc, s, 0, len, epos, elen);
  return run_record<F_LINE>(acc, s, 0, len, epos, elen);
}
// what a validated record leaves in its row (one lane): the length; or the node's terminator, the
// FASTA piece in the row itself (rows at and after a node's terminator are not part of its table)
__device__ __forceinline__ void b_settle(const BatchArgs &p, u64 i, u64 r, u64 k, u32 st, u64 len, u64 epos, u64 elen) {
  if (st == ST_OK) {
    p.rows[2 * r + 1] = len;
    return;
  }
  if (st == ST_DEFER) {
    p.rows[2 * r + 1] = B_DEFER;
    return;
  }
  p.rows[2 * r + 1] = 0;
  if (st == ST_FA_INVALID) {
    p.rows[2 * r] = epos;
    p.rows[2 * r + 1] = elen;
  }
  atomicMin((unsigned long long *)&p.key[i], (unsigned long long)((k << 4) | st));
}

__global__ __launch_bounds__(256) void k_b_check(const BatchArgs p) {
  if (!p.ctl[BC_GO]) return;
  const u64 total = p.ctl[BC_TOTAL];
  for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += (u64)gridDim.x * blockDim.x) {
    const u64 i = b_node_of_row(p.base, p.K, r);
    const BNode nd = b_node(p, i);
    if (!nd.batched) continue;
    NodeAcc acc{nd.g, nd.len, 1, 0};
    const u64 k = r - p.base[i], s = p.rows[2 * r];
    u64 len = 0, epos = 0, elen = 0;
    const u32 st = b_validate(acc, nd.fmt, k, s, len, epos, elen);
    b_settle(p, i, r, k, st, len, epos, elen);
  }
}

__global__ __launch_bounds__(256) void k_b_fix(const BatchArgs p) {
  if (!p.ctl[BC_GO]) return;
  const int lane = threadIdx.x & 63;
  const u64 total = p.ctl[BC_TOTAL];
  const u64 nw = (u64)gridDim.x * (blockDim.x / 64);
  for (u64 c = (u64)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); c * 64 < total; c += nw) {
    const u64 mine = c * 64 + lane;
    u64 todo = __ballot(mine < total && p.rows[2 * mine + 1] == B_DEFER);
    for (; todo; todo &= todo - 1) {
      const u64 r = c * 64 + ctz64(todo);
      const u64 i = b_node_of_row(p.base, p.K, r);
      const BNode nd = b_node(p, i);
      if (!nd.batched) continue;  // (a single's region: its build has not run yet)
      WaveAcc wa;
      wa.g = nd.g; wa.end = nd.len; wa.eof = 1; wa.lane = lane; wa.front = 0;
      const u64 k = r - p.base[i], s = p.rows[2 * r];
      u64 len = 0, epos = 0, elen = 0;
      const u32 st = b_validate(wa, nd.fmt, k, s, len, epos, elen);
      if (lane == 0) b_settle(p, i, r, k, st, len, epos, elen);
    }
  }
}

// The end-of-build invariants of the single build's finalize (record.go:51-83), over one node's
// finished table: row 0 at 0, every row starting where the previous one ends, and after a build that
// no error ended the last row ending at the node's end -- a FASTQ build may leave blank lines behind
// it, and the line index's last row is what follows the last '\n'.
__device__ bool b_table_bad(const BatchArgs &p, const BNode &nd, u64 r0, u64 count, u32 code) {
  if (!count) return false;
  const u64 *rw = p.rows + 2 * r0;
  bool bad = rw[0] != 0;
  for (u64 j = 0; j + 1 < count; ++j) bad |= rw[2 * j] + rw[2 * j + 1] != rw[2 * (j + 1)];
  if (code == ST_OK || code == ST_END || code == ST_ABSENT) {
    const u64 e = rw[2 * (count - 1)] + rw[2 * (count - 1) + 1], fe = nd.len;
    if (nd.fmt == F_FASTQ) bad |= e > fe || (e < fe && (nd.g[e] != '\n' || nd.g[fe - 1] != '\n'));
    else bad |= e != fe;
    if (nd.fmt == F_LINE) bad |= rw[2 * (count - 1) + 1] != 0 && fe && nd.g[fe - 1] == '\n';
  }
  return bad;
}

__global__ __launch_bounds__(256) void k_b_finish(const BatchArgs p) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.K || !p.ctl[BC_GO]) return;
  const BNode nd = b_node(p, i);
  BatchItem it = {};
  it.row_off = p.base[i];
  it.format = nd.fmt;
  if (!batch_is_small(nd.len, p.small)) {  // a single: the host fills the rest in from its build
    p.items[i] = it;
    return;
  }
  it.path = BATCH_PATH;
  if (nd.fmt == F_NONE) {  // errors.go:20 via multi.go:61: "Invalid file type for filter"
    it.status = SHOCKIDX_EFORMAT;
    p.items[i] = it;
    return;
  }
  const u64 key = p.key[i], nat = p.nat[i];
  u32 code = ST_OK;
  it.count = nat;
  if (key != ~0ull) {
    it.count = key >> 4;
    code = (u32)(key & 15);
    if (code == ST_FA_INVALID) {
      it.err_pos = p.rows[2 * (it.row_off + it.count)];
      it.err_len = p.rows[2 * (it.row_off + it.count) + 1];
    }
  }
  it.term_code = code;
  const bool fine = code == ST_OK || code == ST_END || code == ST_ABSENT;
  it.status = fine ? 0 : SHOCKIDX_EFORMAT;
  bool internal = code == ST_DONTCARE || code == ST_NEEDMORE || code == ST_DEFER || code == ST_SLOW || it.count > nat;
  if (p.verify && !internal) internal = b_table_bad(p, nd, it.row_off, it.count, code);
  if (internal) atomicOr((unsigned long long *)&p.ctl[BC_INTERNAL], 1ull);
  else if (fine) atomicAdd((unsigned long long *)&p.ctl[BC_NOK], 1ull);
  p.items[i] = it;
}

}  // namespace sidx

using namespace sidx;

// wave-per-node kernels: four nodes per workgroup, at most this many workgroups (the nodes beyond
// 4 * B_WAVE_GRID_MAX are taken by the grid stride)
constexpr u32 B_WAVE_GRID_MAX = 2048;
static u32 b_wave_grid(u64 n) { return (u32)((n + 3) / 4 < B_WAVE_GRID_MAX ? (n + 3) / 4 : B_WAVE_GRID_MAX); }
constexpr u64 B_LANE_GRID_MAX = 1u << 20;  // lane-per-record grid (rows beyond it: the grid stride)
static u32 b_lane_grid(u64 n) { return (u32)((n + 255) / 256); }

// the range check, the singles and the slot reset; ctl zeroed by the caller.  One launch.
extern "C" hipError_t sidx_batch_classify(const BatchArgs *p, hipStream_t s) {
  hipLaunchKernelGGL(k_b_classify, dim3(b_lane_grid(p->K)), dim3(256), 0, s, *p);
  return hipGetLastError();
}
// nat[i] for every node (nfmt is final).  One launch.
extern "C" hipError_t sidx_batch_count(const BatchArgs *p, hipStream_t s) {
  hipLaunchKernelGGL(k_b_count, dim3(b_wave_grid(p->K)), dim3(256), 0, s, *p);
  return hipGetLastError();
}
// After the scan of nat into base: the layout, the candidate starts, the checks, the marked records
// and the items.  total_bound: a bound on the table's rows the host can know (row_cap: nothing is
// written beyond it).  *launches += the kernels launched.
extern "C" hipError_t sidx_batch_index(const BatchArgs *p, u64 total_bound, u32 *launches, hipStream_t s) {
  hipLaunchKernelGGL(k_b_layout, dim3(1), dim3(64), 0, s, *p);
  hipLaunchKernelGGL(k_b_emit, dim3(b_wave_grid(p->K)), dim3(256), 0, s, *p);
  *launches += 2;
  if (total_bound) {
    const u64 nb = (total_bound + 255) / 256;
    hipLaunchKernelGGL(k_b_check, dim3((u32)(nb < B_LANE_GRID_MAX ? nb : B_LANE_GRID_MAX)), dim3(256), 0, s, *p);
    hipLaunchKernelGGL(k_b_fix, dim3(b_wave_grid((total_bound + 63) / 64)), dim3(256), 0, s, *p);
    *launches += 2;
  }
  hipLaunchKernelGGL(k_b_finish, dim3(b_lane_grid(p->K)), dim3(256), 0, s, *p);
  *launches += 1;
  return hipGetLastError();
}
