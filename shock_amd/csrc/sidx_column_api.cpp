// sidx_column_api.cpp -- the column index entry points of the C ABI (index/column.go:33-130,
// called from node/index.go:43-54) over sidx_column.hip: the tile pass, or the general build
// over the line index of the bytes.
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
  if (int rc = stage_fd(c, fd, 0, n, c->stream, res)) return rc;
  if (int rc = column_build(c, c->d_in, n, (u32)column, true, nullptr, 0, c->stream, res)) return rc;
  if (int rc = fetch_rows(c, res->count, c->stream, rows, res)) return rc;
  res->total_ms = now_ms() - t0;
  return SHOCKIDX_OK;
}

}  // extern "C"
