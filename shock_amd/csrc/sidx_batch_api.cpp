// sidx_batch_api.cpp -- the batch build of the C ABI: many small nodes of one arena indexed in one
// call, over the kernels of sidx_batch.hip.  Node i's result is shockidx_build_device's over its
// bytes alone (include/shockidx.h, "The batch build").
//
// The device call classifies the nodes on the device.  Every node of at most SHOCKIDX_BATCH_SMALL
// bytes, whatever its format, is indexed by the batched walk: classify, per-node detection (AUTO),
// count, the scan that places the row regions, then layout / emit / check / fix / finish -- a fixed
// list of launches, and two host waits (the control words, then the items and the singles), neither
// of which grows with the list.  Nodes longer than the limit ("singles") go through run_index on
// d_data + pos, one at a time in list order, into their region of the same table, whose size the
// count pass has fixed for them too.  pure arithmetic: sidx_batch_host.hpp.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/shockidx.h"
#include "sidx_batch.hpp"
#include "sidx_batch_host.hpp"
#include "sidx_common.hpp"
#include "sidx_host.hpp"
#include "sidx_launch.hpp"

using namespace sidx;
using namespace sidx_host;

static_assert(sizeof(shockidx_batch_item) == sizeof(BatchItem), "the device writes shockidx_batch_item");
static_assert(offsetof(shockidx_batch_item, err_pos) == offsetof(BatchItem, err_pos), "the device writes shockidx_batch_item");

namespace {

// Nodes at most this long take the batched walk (SHOCKIDX_BATCH_SMALL, bytes; DESIGN.md, "The batch
// build").  A lane validates a whole record and a wave walks a whole node, so the walk is for nodes
// of a few tiles; past that the tile passes, which spread one node over the whole grid, are faster.
constexpr u64 BATCH_SMALL_DEFAULT = 256ull << 10;

u64 round256(u64 v) { return (v + 255) / 256 * 256; }

const char NO_FORMAT[] = "Invalid file type for filter";  // errors.go:20 via multi.go:61

// the kernel format of the whole batch (F_NONE: detect per node), or < 0
int batch_format(int kind, int fmt, Err res) {
  if (kind == SHOCKIDX_LINE) return F_LINE;
  if (kind != SHOCKIDX_RECORD) return set_msg(res, SHOCKIDX_EINVAL, "invalid index kind");
  if (fmt == SHOCKIDX_FMT_AUTO) return F_NONE;
  if (fmt != SHOCKIDX_FMT_FASTA && fmt != SHOCKIDX_FMT_FASTQ && fmt != SHOCKIDX_FMT_SAM && fmt != SHOCKIDX_FMT_LINE)
    return set_msg(res, SHOCKIDX_EINVAL, "invalid format");
  return fmt;
}

// one single: the existing build over the node's bytes into its region of the table
int run_single(shockidx_ctx *c, const uint8_t *dd, const BatchSingle &sg, u64 *d_rows, u64 region,
               shockidx_batch_item *it, shockidx_result *res) {
  it->path = 0;
  if (it->format == SHOCKIDX_FMT_NONE) {
    it->status = SHOCKIDX_EFORMAT;
    return 0;
  }
  shockidx_result r;
  reset_result(&r);
  DevResult dr;
  if (int rc = run_index(c, dd + sg.pos, (u64)sg.len, it->format, d_rows + 2 * it->row_off, region, c->stream, &dr, &r)) {
    forward_error(res, r, rc);
    return rc;
  }
  c->batch_stats.launches += 1 + r.reruns;
  c->batch_stats.waits += 1 + r.reruns;
  res->kernel_ms += r.kernel_ms;
  if (dr.flags & (RF_INTERNAL | RF_HALO | RF_CAPACITY))
    return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: device invariant violated");
  it->count = dr.count;
  it->term_code = dr.code;
  it->path = r.path;
  it->err_pos = dr.err_pos;
  it->err_len = dr.err_len;
  const bool fine = dr.code == ST_OK || dr.code == ST_END || dr.code == ST_ABSENT;
  if (!fine && dr.code != ST_FA_INVALID && !status_message(dr.code))
    return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: unknown device status");
  it->status = fine ? SHOCKIDX_OK : SHOCKIDX_EFORMAT;
  return 0;
}

}  // namespace

extern "C" {

int shockidx_build_batch_device(shockidx_ctx *c, const void *d_data, uint64_t data_len, const void *d_nodes,
                                uint64_t nnodes, int kind, int fmt, void *d_rows, uint64_t row_cap,
                                shockidx_batch_item *items, uint64_t *rows_total, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (rows_total) *rows_total = 0;
  if (!c || (!d_data && data_len) || ((uintptr_t)d_data & 15) || (!d_nodes && nnodes) || ((uintptr_t)d_nodes & 7) ||
      (!items && nnodes) || (!d_rows && row_cap) || ((uintptr_t)d_rows & 15) || nnodes > (1ull << 40))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const int bfmt = batch_format(kind, fmt, res);
  if (bfmt < 0) return bfmt;
  res->format = bfmt;
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  c->batch_stats = shockidx_batch_stats{};
  c->batch_stats.nodes = nnodes;
  if (!nnodes) return SHOCKIDX_OK;
  const u64 K = nnodes;
  const uint8_t *dd = (const uint8_t *)d_data;

  size_t sb = 0;
  HIPCHK(sidx_scan_u64(nullptr, nullptr, K, nullptr, &sb, s), "scan size");
  if (int rc = c->d_batch.ensure(round256(8 * BC_NWORDS) + round256(4 * K) + 3 * round256(8 * K) +
                                     round256(sizeof(BatchSingle) * K) + round256(sizeof(BatchItem) * K) + round256(sb) + 4096,
                                 res))
    return rc;
  Carver ca{c->d_batch};
  BatchArgs p;
  memset(&p, 0, sizeof p);
  p.data = dd;
  p.data_len = data_len;
  p.nodes = (const i64 *)d_nodes;
  p.K = K;
  p.small = batch_small_limit(getenv("SHOCKIDX_BATCH_SMALL"), BATCH_SMALL_DEFAULT);
  p.fmt = bfmt;
  p.verify = verify_rows() ? 1 : 0;
  p.ctl = ca.take<u64>(BC_NWORDS);
  p.nfmt = ca.take<int>(K);
  p.nat = ca.take<u64>(K);
  p.base = ca.take<u64>(K);
  p.key = ca.take<u64>(K);
  p.singles = ca.take<BatchSingle>(K);
  p.items = ca.take<BatchItem>(K);
  void *stmp = ca.take<uint8_t>(sb);
  p.rows = (u64 *)d_rows;
  p.row_cap = row_cap;

  u64 w[BC_NWORDS];
  std::vector<BatchSingle> singles;
  u32 launches = 0;
  {
    // the batched walk's device work, like every build's: one at a time per GPU
    std::unique_lock<std::mutex> device_lock(device_mutex(c->device));
    HIPCHK(hipEventRecord(c->ek0, s), "event");
    HIPCHK(hipMemsetAsync(p.ctl, 0, 8 * BC_NWORDS, s), "memset");
    HIPCHK(sidx_batch_classify(&p, s), "batch classify");
    launches += 1;
    if (bfmt == F_NONE) {  // multi.DetermineFormat once per node (a node outside the arena reads nothing)
      HIPCHK(sidx_launch_detect_sections(dd, data_len, d_nodes, K, p.nfmt, s), "detect launch");
      launches += 1;
    }
    HIPCHK(sidx_batch_count(&p, s), "batch count");
    HIPCHK(sidx_scan_u64(p.nat, p.base, K, stmp, &sb, s), "scan");
    launches += 1 + (K <= sidx_scan_small_items() ? 3 : 1);
    HIPCHK(sidx_batch_index(&p, row_cap, &launches, s), "batch index");
    HIPCHK(hipEventRecord(c->ek1, s), "event");
    HIPCHK(hipMemcpyAsync(w, p.ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
    HIPCHK(hipStreamSynchronize(s), "control sync");
    c->batch_stats.launches = launches;
    c->batch_stats.waits = 1;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
    res->kernel_ms += ms;
    if (w[BC_INVALID]) return set_msg(res, SHOCKIDX_EINVAL, "node outside the data or not 16-byte aligned");
    if (rows_total) *rows_total = w[BC_TOTAL];
    if (!w[BC_GO]) return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
    if (w[BC_INTERNAL] || w[BC_NSINGLE] > K || w[BC_TOTAL] > row_cap)
      return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: device invariant violated");
    singles.resize(w[BC_NSINGLE]);
    HIPCHK(hipMemcpyAsync(items, p.items, sizeof(BatchItem) * K, hipMemcpyDeviceToHost, s), "items copy");
    if (!singles.empty())
      HIPCHK(hipMemcpyAsync(singles.data(), p.singles, sizeof(BatchSingle) * singles.size(), hipMemcpyDeviceToHost, s),
             "singles copy");
    HIPCHK(hipStreamSynchronize(s), "items sync");
    c->batch_stats.waits += 1;
  }
  BatchSplit split;
  if (!batch_split(K, singles.size(), &split)) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: batch split");
  c->batch_stats.batches = split.batches;
  c->batch_stats.batched = split.batched;
  c->batch_stats.singles = split.singles;

  // the singles in list order (the classify kernel appends them in any order)
  std::sort(singles.begin(), singles.end(), [](const BatchSingle &a, const BatchSingle &b) { return a.node < b.node; });
  u64 nok = w[BC_NOK];
  for (const BatchSingle &sg : singles) {
    if (sg.node >= K) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: batch singles");
    shockidx_batch_item *it = &items[sg.node];
    const u64 next = sg.node + 1 < K ? items[sg.node + 1].row_off : w[BC_TOTAL];
    if (int rc = run_single(c, dd, sg, (u64 *)d_rows, batch_region_rows(it->row_off, next, w[BC_TOTAL]), it, res)) return rc;
    nok += it->status == SHOCKIDX_OK;
  }
  for (u64 i = 0; i < K; ++i) {
    const int f = items[i].format;
    if (f == F_FASTQ || f == F_FASTA || f == F_SAM || f == F_LINE)
      c->batch_stats.by_format[f == F_FASTQ ? 0 : f == F_FASTA ? 1 : f == F_SAM ? 2 : 3] += 1;
  }
  res->count = nok;
  res->path = BATCH_PATH;
  res->total_ms = now_ms() - t0;
  return SHOCKIDX_OK;
}

int shockidx_build_batch_host(shockidx_ctx *c, const void *const *bodies, const uint64_t *lens, uint64_t nnodes,
                              int kind, int fmt, uint64_t **rows, shockidx_batch_item *items, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !rows || ((!bodies || !lens || !items) && nnodes) || nnodes > (1ull << 40))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  for (u64 i = 0; i < nnodes; ++i)
    if (!bodies[i] && lens[i]) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const u64 K = nnodes;
  std::vector<uint64_t> pos(K ? K : 1);
  uint64_t arena = 0, cap = 0;
  if (!batch_pack(lens, K, pos.data(), &arena) || !batch_rows_guess(arena, K, &cap))
    return set_msg(res, SHOCKIDX_EINVAL, "batch too large");
  std::vector<i64> nodes(2 * (K ? K : 1));
  for (u64 i = 0; i < K; ++i) {
    nodes[2 * i] = (i64)pos[i];
    nodes[2 * i + 1] = (i64)lens[i];
  }
  // the arena through the pinned staging, chunk by chunk: each chunk is the bodies (and the zeroed
  // padding between them) that fall into it
  const double th = now_ms();
  if (int rc = c->d_in.ensure(arena + 64, res)) return rc;
  if (int rc = c->d_bnodes.ensure(16 * K + 64, res)) return rc;
  {
    u64 first = 0;  // the first node that reaches into the chunk
    int b = 0;
    for (u64 off = 0; off < arena; off += STAGE_BYTES, b ^= 1) {
      const u64 k = arena - off < STAGE_BYTES ? arena - off : STAGE_BYTES;
      HIPCHK(hipEventSynchronize(c->stage_ev[b]), "stage wait");
      uint8_t *dst = c->h_stage[b];
      memset(dst, 0, k);
      while (first < K && pos[first] + lens[first] <= off) ++first;
      for (u64 i = first; i < K && pos[i] < off + k; ++i) {
        const u64 lo = pos[i] > off ? pos[i] : off, hi = pos[i] + lens[i] < off + k ? pos[i] + lens[i] : off + k;
        if (hi > lo) memcpy(dst + (lo - off), (const uint8_t *)bodies[i] + (lo - pos[i]), hi - lo);
      }
      HIPCHK(hipMemcpyAsync(c->d_in + off, dst, k, hipMemcpyHostToDevice, s), "H2D");
      HIPCHK(hipEventRecord(c->stage_ev[b], s), "stage event");
    }
    if (K) HIPCHK(hipMemcpyAsync(c->d_bnodes.get(), nodes.data(), 16 * K, hipMemcpyHostToDevice, s), "H2D");
    HIPCHK(hipStreamSynchronize(s), "H2D sync");
  }
  const double h2d = now_ms() - th;
  uint64_t total = 0;
  int rc = SHOCKIDX_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (int rc2 = c->d_rows.ensure(cap, res)) return rc2;
    rc = shockidx_build_batch_device(c, c->d_in.get(), arena, c->d_bnodes.get(), K, kind, fmt, c->d_rows.get(),
                                     c->d_rows.cap, items, &total, res);
    if (rc != SHOCKIDX_ESPACE) break;
    cap = total;  // what the call said it needs
  }
  if (rc != SHOCKIDX_OK) return rc;
  res->h2d_ms = h2d;
  const double td = now_ms();
  const size_t bytes = (size_t)total * 16;
  uint64_t *out = alloc_rows_out(bytes);
  if (!out) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
  if (int rc2 = rows_to_host(c, c->d_rows, bytes, (uint8_t *)out, s, res)) {
    free(out);
    return rc2;
  }
  *rows = out;
  res->d2h_ms = now_ms() - td;
  res->total_ms = now_ms() - t0;
  return SHOCKIDX_OK;
}

int shockidx_batch_error(shockidx_ctx *c, const void *d_data, const shockidx_batch_item *item, const void *node,
                         char *buf, uint64_t cap, uint64_t *len) {
  if (len) *len = 0;
  if (!c || !item || !node || (!buf && cap)) return SHOCKIDX_EINVAL;
  shockidx_result r;
  reset_result(&r);
  if (item->status == SHOCKIDX_OK) return SHOCKIDX_OK;
  if (item->status != SHOCKIDX_EFORMAT) return SHOCKIDX_EINVAL;
  int rc;
  if (item->format == SHOCKIDX_FMT_NONE) {
    rc = set_msg(&r, SHOCKIDX_EFORMAT, NO_FORMAT);
  } else if (item->term_code == ST_FA_INVALID) {
    i64 pl[2];
    memcpy(pl, node, sizeof pl);
    const uint8_t *dd = d_data ? (const uint8_t *)d_data : c->d_in.get();
    if (!dd || pl[0] < 0 || pl[1] < 0 || item->err_pos > (u64)pl[1] || item->err_len > (u64)pl[1] - item->err_pos)
      return SHOCKIDX_EINVAL;
    Err res(&r);
    HIPCHK(hipSetDevice(c->device), "hipSetDevice");
    rc = fasta_error_text(res, item->err_len, [&](char *dst, u64 k) -> int {
      hipError_t e = hipMemcpyAsync(dst, dd + pl[0] + item->err_pos, k, hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      return e == hipSuccess ? 0 : set_hip(res, e, "error text copy");
    });
  } else {
    const char *m = status_message(item->term_code);
    if (!m) return SHOCKIDX_EINTERNAL;
    rc = set_msg(&r, SHOCKIDX_EFORMAT, m);
  }
  if (rc != SHOCKIDX_EFORMAT) return rc;
  const u64 k = r.err_len < cap ? r.err_len : cap;
  if (k) memcpy(buf, r.err, k);
  if (len) *len = k;
  return SHOCKIDX_OK;
}

int shockidx_batch_last_stats(const shockidx_ctx *c, shockidx_batch_stats *out) {
  if (!c || !out) return SHOCKIDX_EINVAL;
  *out = c->batch_stats;
  return SHOCKIDX_OK;
}

}  // extern "C"
