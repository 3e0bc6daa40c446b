// sidx_column_api.cpp -- the column index entry points of the C ABI (index/column.go:33-130,
// called from node/index.go:43-54) over sidx_column.hip: the tile pass, or the general build
// over the line index of the bytes; and the same loop (column.go:53-108) one slab at a time, its
// state (column.go:44-48) in a device carry, for nodes that do not fit the device budget.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_launch.hpp"
#include "sidx_host.hpp"

using namespace sidx;
using namespace sidx_host;

namespace {

// column.go:76
const char COLUMN_MISSING[] = "Specified column does not exist for all lines in file.";

// SHOCKIDX_COLUMN_MODE=two (or 0): the general build instead of the tile pass; read per build
bool forced_general() {
  const char *e = getenv("SHOCKIDX_COLUMN_MODE");
  return e && (!strcmp(e, "two") || !strcmp(e, "0"));
}

// The general build up to its cuts: the line index into c->d_cola, sidx_col_cuts over it.
// *ctl: the device control words; the cut offsets are left in c->d_cola.
int general_cuts(shockidx_ctx *c, const uint8_t *dd, u64 n, u32 column, hipStream_t s, const u64 **ctl_out,
                 shockidx_result *res) {
  // the line index (line.go:33-85): one row per ReadBytes('\n') piece, the last possibly empty
  u64 lcap = n / 16 + 4096, L = 0;
  for (int attempt = 0;; ++attempt) {
    if (attempt == 3) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: row capacity");
    if (int rc = c->d_cola.ensure(lcap * 16, res)) return rc;
    DevResult dr;
    shockidx_result r2;
    reset_result(&r2);
    if (int rc = run_index(c, dd, n, F_LINE, c->d_cola.as<u64>(), lcap, s, &dr, &r2)) return forward_error(res, r2, rc);
    res->kernel_ms += r2.kernel_ms;
    if (dr.flags & RF_CAPACITY) {
      lcap = dr.count;
      res->reruns++;
      continue;
    }
    if ((dr.flags & (RF_INTERNAL | RF_HALO)) || !dr.count)
      return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: device invariant violated");
    L = dr.count;
    break;
  }
  const u64 sb = sidx_col_scan_bytes(L);
  if (int rc = c->d_colb.ensure(256 + (4 + 8 + sizeof(ColKey)) * L + sb + 4 * 256, res))
    return rc;
  Carver cv{c->d_colb};
  u64 *ctl = cv.take<u64>(COL_CTL_WORDS);
  u32 *flag = cv.take<u32>(L);
  u64 *rank = cv.take<u64>(L);
  ColKey *ck = cv.take<ColKey>(L);
  void *scan_tmp = cv.take<uint8_t>(sb);
  *ctl_out = ctl;
  HIPCHK(hipEventRecord(c->ev0, s), "event");
  HIPCHK(sidx_col_cuts(dd, n, c->d_cola.as<u64>(), L, column, flag, rank, ck, ctl, scan_tmp, sb, s), "column launch");
  return 0;
}

// One build.  own: the table goes to c->d_rows, grown to the row count (the fd entry point);
// else to d_rows / row_cap.
int column_build(shockidx_ctx *c, const uint8_t *dd, u64 n, u32 column, bool own, u64 *d_rows, u64 row_cap,
                 hipStream_t s, shockidx_result *res) {
  const bool tiles = !forced_general();
  res->path = tiles ? 1 : 2;
  if (!n) return SHOCKIDX_OK;  // one empty piece, blank: no rows (column.go:64-68,119)
  const u64 *ctl = nullptr;
  if (tiles) {
    const u64 nt = (n + TILE - 1) / TILE;
    if (int rc = c->d_colb.ensure(sidx_col_tile_bytes(nt), res)) return rc;
    HIPCHK(hipEventRecord(c->ev0, s), "event");
    HIPCHK(sidx_col_tile_cuts(dd, n, column, c->tiles_grid, c->d_colb, &ctl, s), "column tile pass launch");
  } else if (int rc = general_cuts(c, dd, n, column, s, &ctl, res)) {
    return rc;
  }
  HIPCHK(hipMemcpyAsync(c->h_det, ctl, COL_CTL_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s), "column copy");
  HIPCHK(hipStreamSynchronize(s), "column sync");
  u64 h[COL_CTL_WORDS];
  memcpy(h, c->h_det, sizeof h);
  if (h[COL_BAD] != ~0ull) return set_msg(res, SHOCKIDX_EFORMAT, COLUMN_MISSING);
  const u64 B = h[COL_B], count = B ? B + 1 : 0;
  if (own) {
    if (int rc = c->d_rows.ensure(count ? count : 1, res)) return rc;
    d_rows = c->d_rows;
    row_cap = c->d_rows.cap;
  }
  res->count = count;
  if (count > row_cap) return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  if (count) {
    if (tiles) HIPCHK(sidx_col_tile_rows(n, c->d_colb, count, d_rows, row_cap, s), "column rows launch");
    else HIPCHK(sidx_col_rows(c->d_cola.as<u64>(), ctl, B, n, d_rows, row_cap, s), "column rows launch");
    HIPCHK(hipEventRecord(c->ev1, s), "event");
    if (verify_rows()) {  // SHOCKIDX_VERIFY: contiguous rows from 0 to n
      DevResult *d_res = (DevResult *)(c->d_small + SMALL_RESULT);
      HIPCHK(sidx_col_check(d_rows, count, n, d_res, s), "column check launch");
      HIPCHK(sidx_launch_verify_rows(d_rows, 0, row_cap, d_res, s), "verify launch");
      HIPCHK(hipMemcpyAsync(c->h_res, d_res, sizeof(DevResult), hipMemcpyDeviceToHost, s), "result copy");
    }
    HIPCHK(hipStreamSynchronize(s), "column sync");
    if (verify_rows() && (c->h_res->flags & RF_INTERNAL)) {
      res->count = 0;
      return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: device invariant violated");
    }
  } else {
    HIPCHK(hipEventRecord(c->ev1, s), "event");
    HIPCHK(hipEventSynchronize(c->ev1), "event sync");
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  res->kernel_ms += ms;
  res->index_ms = res->kernel_ms;
  return SHOCKIDX_OK;
}

}  // namespace

namespace sidx_host {

u64 column_whole_bytes(u64 n) {
  const u64 node = n + 64, tb = sidx_col_tile_bytes((n + TILE - 1) / TILE), rows = 16 * (n / 32 + 4096);
  return node + node / 8 + tb + tb / 8 + rows + rows / 8 + (1ull << 20);
}

// column.go:64-101 over one slab: the tile pass bounded by the slab's window, one host stop (the
// first line without the column, the first line the window cannot settle, the rows), then the
// rows against the carried cut and the carry for the next slab.
int column_slab_run(shockidx_ctx *c, const ColSlabIn &sl, u32 column, void *ws, ColCarry *carry, u64 *d_rows,
                    u64 row_cap, hipStream_t s, shockidx_result *res) {
  res->path = 5;
  res->format = SHOCKIDX_FMT_LINE;
  ColSlabArgs sa;
  memset(&sa, 0, sizeof sa);
  sa.end = sl.end;
  sa.base = sl.base;
  sa.file_size = sl.file_size;
  sa.carry = carry;
  sa.eof = sl.base + sl.end == sl.file_size;
  sa.first = sl.first;
  sa.last = sl.last;
  const u64 *ctl = nullptr;
  HIPCHK(hipEventRecord(c->ev0, s), "event");
  HIPCHK(sidx_col_slab_cuts(sl.d, sl.n, sl.front, &sa, column, c->tiles_grid, ws, &ctl, s), "column slab launch");
  HIPCHK(hipMemcpyAsync(c->h_det, ctl, COL_SLAB_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s), "column copy");
  HIPCHK(hipStreamSynchronize(s), "column sync");
  u64 h[COL_SLAB_WORDS];
  memcpy(h, c->h_det, sizeof h);
  // the earlier of the two lines decides (a bad line after an unsettled one may be the unsettled
  // line's own tail)
  if (h[COLS_MORE] != ~0ull && h[COLS_MORE] < h[COL_BAD]) {
    res->state_out = sl.base + h[COLS_MORE];
    return set_msg(res, SHOCKIDX_EMORE, "a line of the slab does not close inside its window");
  }
  if (h[COL_BAD] != ~0ull) return set_msg(res, SHOCKIDX_EFORMAT, COLUMN_MISSING);
  const u64 nrows = h[COLS_ROWS];
  res->count = nrows;
  if (nrows > row_cap) return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  HIPCHK(sidx_col_slab_rows(sl.d, sl.n, &sa, ws, carry, d_rows, nrows, s), "column rows launch");
  HIPCHK(hipEventRecord(c->ev1, s), "event");
  HIPCHK(hipStreamSynchronize(s), "column sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  res->kernel_ms += ms;
  res->index_ms = res->kernel_ms;
  return SHOCKIDX_OK;
}

}  // namespace sidx_host

extern "C" {

// CreateColumnIndex (index/column.go:33-130).  The first non-blank line with fewer than `column`
// fields is SHOCKIDX_EFORMAT with column.go:76's text: the reference returns that error when
// len(slices) < column-1 (:75) and panics with index out of range at slices[column-1] (:79) when
// len(slices) == column-1; both are the error here.  Default: the tile pass (sidx_column.hip,
// result->path 1); SHOCKIDX_COLUMN_MODE=two: the general build over the line index (path 2), kept
// as a tested path.
int shockidx_column_device(shockidx_ctx *c, const void *d_data, uint64_t n, int column, void *d_rows,
                           uint64_t row_cap, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  res->format = SHOCKIDX_FMT_LINE;
  if (!c || (!d_data && n) || (!d_rows && row_cap) || column < 1) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  const int rc = column_build(c, (const uint8_t *)d_data, n, (u32)column, false, (u64 *)d_rows, row_cap, c->stream, res);
  res->total_ms = now_ms() - t0;
  return rc;
}

// the column index over an open file: every byte to HBM through the pinned pread staging, the
// table back to a malloc'ed array
int shockidx_column_fd(shockidx_ctx *c, int fd, uint64_t n, int column, uint64_t **rows, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  res->format = SHOCKIDX_FMT_LINE;
  if (!c || !rows || fd < 0 || column < 1) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  TrimGuard trim{c};
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  if (column_whole_bytes(n) > dev_budget(c)) return shockidx_column_fd_walk(c, fd, n, column, 0, 0, rows, res);
  if (int rc = stage_fd(c, fd, 0, n, c->stream, res)) return rc;
  if (int rc = column_build(c, c->d_in, n, (u32)column, true, nullptr, 0, c->stream, res)) return rc;
  if (int rc = fetch_rows(c, res->count, c->stream, rows, res)) return rc;
  res->total_ms = now_ms() - t0;
  return SHOCKIDX_OK;
}

uint64_t shockidx_column_carry_bytes(void) { return sizeof(ColCarry); }

// One slab of the column index (column.go:64-101 with its loop state carried from slab to slab).
int shockidx_column_slab_device(shockidx_ctx *c, const shockidx_slab *slab, uint64_t file_size, int column,
                                void *d_carry, void *d_rows, uint64_t row_cap, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  res->format = SHOCKIDX_FMT_LINE;
  if (!c || !slab || !d_carry || (!d_rows && row_cap) || column < 1) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const shockidx_slab &b = *slab;
  const bool first = b.base == 0, last = b.base + b.n == file_size;
  if (b.end < b.n || b.base > file_size || b.end > file_size - b.base || (!b.n && file_size) ||
      (b.n && (!b.d_data || ((uintptr_t)b.d_data & 15))) || (b.is_first != 0) != first || (b.is_last != 0) != last ||
      (b.front < 16 && b.base >= 16) || b.front > b.base || ((uintptr_t)d_carry & 7))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  const u64 nt = (b.n + TILE - 1) / TILE;
  if (int rc = c->d_colb.ensure(sidx_col_tile_bytes(nt ? nt : 1), res)) return rc;
  const ColSlabIn sl{(const uint8_t *)b.d_data, b.n, b.end, b.front, b.base, file_size, first, last};
  const int rc = column_slab_run(c, sl, (u32)column, c->d_colb, (ColCarry *)d_carry, (u64 *)d_rows, row_cap, c->stream, res);
  res->total_ms = now_ms() - t0;
  return rc;
}

// The slab walk over an open descriptor, whatever the node's size: the table back to a malloc'ed
// array (result->path 5).
int shockidx_column_fd_walk(shockidx_ctx *c, int fd, uint64_t n, int column, uint64_t slab_bytes, uint64_t halo_bytes,
                            uint64_t **rows, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  res->format = SHOCKIDX_FMT_LINE;
  if (!c || !rows || fd < 0 || column < 1) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  TableSink sink(n / 64);  // (a row per cut, not per line: a table this size is rare)
  if (!sink.out) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
  if (int rc = column_fd_walk(c, fd, n, (u32)column, slab_bytes, halo_bytes, sink, res)) return rc;
  *rows = (uint64_t *)sink.out;
  sink.out = nullptr;
  return SHOCKIDX_OK;
}

}  // extern "C"
