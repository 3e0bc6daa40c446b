// sidx_walks.cpp -- the carried-state walks over a node's file: the column index, the subset
// indexes, the chunkrecord index and the download filters slab by slab through two device slots,
// each loop's state in a device carry, rows to the sink (the filters: bytes to a descriptor) as they
// are made.  sidx_colwalk.hpp, sidx_subwalk.hpp, sidx_chunkwalk.hpp and sidx_filtwalk.hpp hold their
// arithmetic and decisions; the pieces they share with the record
// pipelines (sidx_pipeline.cpp) are declared in sidx_walk.hpp and defined here.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <signal.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <string>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_colwalk.hpp"
#include "sidx_chunkwalk.hpp"
#include "sidx_filtwalk.hpp"
#include "sidx_subwalk.hpp"
#include "sidx_launch.hpp"
#include "sidx_walk.hpp"

using namespace sidx;

namespace sidx_host {

// ---- the shared pieces (sidx_walk.hpp) ---------------------------------------------------------
int walk_prereqs(shockidx_ctx *c, Err res, bool rows) {
  if (!c->s_copy) HIPCHK(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking), "copy stream");
  for (int i = 0; rows && i < 2; ++i)
    if (!c->h_rows[i]) HIPCHK(hipHostMalloc(&c->h_rows[i], STAGE_BYTES, 0), "hipHostMalloc(rows)");
  return 0;
}

int drain_rows(shockidx_ctx *c, const u64 *d_tab, u64 m, u64 first, RowSink &sink, const RowChunkFn &each,
               double *t_d2h, Err res) {
  const double td = now_ms();
  const u64 per = STAGE_BYTES / 16;
  u64 *h = (u64 *)c->h_rows[0];
  for (u64 done = 0; done < m;) {
    const u64 k = m - done < per ? m - done : per;
    HIPCHK(hipMemcpyAsync(h, d_tab + 2 * done, k * 16, hipMemcpyDeviceToHost, c->stream), "rows copy");
    HIPCHK(hipStreamSynchronize(c->stream), "rows copy");
    if (each)
      if (int rc = each(h, k, done)) return rc;
    if (int rc = sink.put(c->h_rows[0], first + done, k, res)) return rc;
    done += k;
  }
  if (t_d2h) *t_d2h += now_ms() - td;
  return 0;
}

int file_to_device(shockidx_ctx *c, int fd, u64 off, u64 total, uint8_t *dst, const char *read_prefix,
                   const char *short_msg, const char *copy_what, Err res) {
  for (u64 done = 0; done < total;) {
    const u64 k = total - done < STAGE_BYTES ? total - done : STAGE_BYTES;
    for (u64 got = 0; got < k;) {
      const ssize_t r = pread(fd, c->h_rows[1] + got, k - got, (off_t)(off + done + got));
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) return set_msg(res, SHOCKIDX_EIO, std::string(read_prefix) + strerror(errno));
      if (r == 0) return set_msg(res, SHOCKIDX_EIO, short_msg);
      got += (u64)r;
    }
    HIPCHK(hipMemcpyAsync(dst + done, c->h_rows[1], k, hipMemcpyHostToDevice, c->stream), copy_what);
    HIPCHK(hipStreamSynchronize(c->stream), copy_what);
    done += k;
  }
  return 0;
}

void finish_walk(shockidx_result *res, int kfmt, u64 total, u32 path, double kernel_ms, double index_ms, double t_d2h,
                 double t0) {
  res->count = total;
  res->format = kfmt == F_LINE ? SHOCKIDX_FMT_LINE : kfmt;
  res->path = path;
  res->kernel_ms = kernel_ms;
  res->index_ms = index_ms;
  res->d2h_ms = t_d2h;
  res->total_ms = now_ms() - t0;
  res->h2d_ms = res->total_ms - t_d2h - res->kernel_ms;
}

namespace {

// a slab of the column layout (sidx_colwalk.hpp) into slot i: its first byte at COLWALK_FRONT
int stage_col(TwoSlots &w, int i, const ColSlabPos &p) {
  return w.stage(i, COLWALK_FRONT - p.front, p.lo - p.front, p.lo + p.end);
}

// a column or chunkrecord slab's m rows into the sink; *next: the offset the table has reached
// (every row starts there: column.go:90-93)
int col_rows_to_sink(shockidx_ctx *c, u64 m, ColRowCursor &cur, u64 *next, RowSink &sink, double *t_d2h,
                     shockidx_result *res) {
  auto contiguous = [&](u64 *r, u64 k, u64) -> int {
    for (u64 i = 0; i < k; ++i) {
      if (r[2 * i] != *next) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_SEAM_MSG);
      *next += r[2 * i + 1];
    }
    return 0;
  };
  return drain_rows(c, c->d_rows, m, cur.take(m), sink, contiguous, t_d2h, res);
}

}  // namespace

// ---- the column index's walk -------------------------------------------------------------------
// CreateColumnIndex (column.go:53-108) slab by slab through two slots: slab k + 1 is copied on the
// copy stream (PageCacheSource: page-cache DMA, else the pinned staging, whose preads run on this
// thread) while slab k's kernels run, each slab's rows go to the sink as they are made, and the
// loop's state travels in the device carry.  sidx_colwalk.hpp holds the sizing and the one retry
// rule.  The device holds the two slots, the carry with one slab's workspace (c->d_colb) and one
// slab's rows, all exact-size.
int column_fd_walk(shockidx_ctx *c, int fd, u64 n, u32 column, u64 S, u64 halo, RowSink &sink, shockidx_result *res) {
  const double t0 = now_ms();
  res->path = 5;
  res->format = SHOCKIDX_FMT_LINE;
  if (!n) return SHOCKIDX_OK;  // one empty piece, blank: no rows (column.go:64-68,119)
  const u64 budget = dev_budget(c);
  const u64 carry_b = (sizeof(ColCarry) + 255) & ~255ull;
  if (!halo) halo = colwalk_default_halo(budget);
  if (halo > n) halo = n;
  if (!S) {
    S = colwalk_slab_bytes(budget, halo, carry_b, sidx_col_tile_bytes);
    if (!S) return set_msg(res, SHOCKIDX_ENOMEM, "device memory: the column walk needs at least 32 MiB of its budget");
  }
  if (S > n) S = n;
  hipStream_t s = c->stream;
  if (int rc = walk_prereqs(c, res)) return rc;
  const u64 slot = colwalk_slot_bytes(S, halo), ws_b = sidx_col_tile_bytes((S + TILE - 1) / TILE);
  u64 row_cap = colwalk_rows_cap(S);
  if (int rc = exact_workspace(c, {{&c->d_slot[0], slot}, {&c->d_slot[1], slot}, {&c->d_colb, carry_b + ws_b}, {&c->d_rows, row_cap}}, res))
    return rc;
  ColCarry *carry = c->d_colb.as<ColCarry>();
  void *ws = c->d_colb + carry_b;
  TwoSlots w(c, fd, 0, n, res);
  HIPCHK(w.events.create(), "event");
  ColRowCursor cur;
  u64 next = 0;
  double t_d2h = 0;
  int i = 0;
  ColSlabPos p = colwalk_slab_at(0, S, halo, n);
  int rc = stage_col(w, 0, p);
  while (!rc) {
    bool more = !p.last;
    ColSlabPos q = p;
    if (more) {  // the slab expected next, on its way while this one is indexed
      q = colwalk_slab_at(p.lo + p.n, S, halo, n);
      if ((rc = stage_col(w, i ^ 1, q))) break;
    }
    if ((rc = w.wait(i))) break;
    shockidx_result r2;
    bool moved = false;
    for (;;) {
      reset_result(&r2);
      const ColSlabIn in{c->d_slot[i] + COLWALK_FRONT, p.n, p.end, p.front, p.lo, n, p.first, p.last};
      rc = column_slab_run(c, in, column, ws, carry, c->d_rows, row_cap, s, &r2);
      res->kernel_ms += r2.kernel_ms;
      if (rc == SHOCKIDX_ESPACE) {  // more cuts than a row per 32 bytes: the rows grow
        row_cap = colwalk_grow_rows(row_cap, r2.count);
        res->reruns++;
        if ((rc = c->d_rows.exact(row_cap, res))) break;
        continue;
      }
      if (rc == SHOCKIDX_EMORE) {  // the retry rule (sidx_colwalk.hpp)
        u64 cut = 0;
        if (colwalk_on_more(p.lo, r2.state_out, &cut) == ColRetry::NoMem) {
          rc = set_msg(res, SHOCKIDX_ENOMEM, "device memory: a line or its key is longer than a slab slot can hold");
          break;
        }
        p = colwalk_shorten(p, cut - p.lo, halo, n);
        q = colwalk_slab_at(cut, S, halo, n);
        more = moved = true;
        res->reruns++;
        continue;
      }
      if (rc) forward_error(res, r2, rc);
      break;
    }
    if (rc) break;
    if ((rc = col_rows_to_sink(c, r2.count, cur, &next, sink, &t_d2h, res))) break;
    if (!more) break;
    if (moved && (rc = stage_col(w, i ^ 1, q))) break;  // a fresh slot from where the shortened slab ends
    p = q;
    i ^= 1;
  }
  if ((rc = w.finish(rc))) {
    res->count = 0;  // (column.go:76 returns count 0; an error leaves no table)
    return rc;
  }
  if (cur.total && next != n) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_END_MSG);
  finish_walk(res, SHOCKIDX_FMT_LINE, cur.total, 5, res->kernel_ms, res->kernel_ms, t_d2h, t0);
  res->status = SHOCKIDX_OK;
  return SHOCKIDX_OK;
}

// ---- the subset indexes' walk ------------------------------------------------------------------
// CreateSubsetNodeIndexes / CreateSubsetIndex (subset.go:186-291) over the two files: the id text
// slab by slab through the two slots (slab k + 1 copied on the copy stream while slab k runs), the
// parent index window by window (pread, as the reference's ReadAt per id: the first window from row
// 0, after a stop at an id the next from that id's row), each call's rows and runs to the sinks as
// they are made, the loop's state in the device carry.  sidx_subwalk.hpp holds the sizing and the
// decisions.  The device holds the two slots, the window, the carry with one slab's runs, one
// call's workspace (c->d_sends, c->d_sub) and one slab's rows, all sized up front.
namespace {

// rows [w.row0, w.row0 + w.rows) of the parent index file into the window buffer
int sub_load_window(shockidx_ctx *c, int fd, const SubWindow &w, Err res) {
  return file_to_device(c, fd, 16 * w.row0, 16 * w.rows, c->d_spar, "read: ",
                        "read: the parent index file is shorter than its size", "window copy", res);
}

}  // namespace

int subset_fd_walk(shockidx_ctx *c, int ids_fd, u64 n, int parent_fd, u64 parent_bytes, i64 ilength, bool want_runs,
                   u64 S, u64 W, SubsetSinks sinks, shockidx_subset_result *res) {
  const double t0 = now_ms();
  shockidx_subset_stats &st = c->subset_stats;
  memset(&st, 0, sizeof st);
  st.walked = 1;
  if (!n) return SHOCKIDX_OK;  // no line: two empty tables (:186-195,274-291)
  const u64 parent_count = parent_bytes / 16, budget = dev_budget(c);
  const u64 carry_b = (sizeof(SubCarry) + 255) & ~255ull;
  u64 halo = SUBWALK_HALO < n ? SUBWALK_HALO : n;
  if (!W) W = subwalk_window_rows(budget, parent_count);
  if (W > parent_count) W = parent_count ? parent_count : 1;
  if (!S) {
    S = subwalk_slab_bytes(budget, halo, W, carry_b, subset_slab_ws_bytes);
    if (!S) return set_msg(res, SHOCKIDX_ENOMEM, "device memory: the subset walk needs at least 32 MiB of its budget");
  }
  if (S > n) S = n;
  st.slab_bytes = S;
  st.window_rows = W;
  hipStream_t s = c->stream;
  if (int rc = walk_prereqs(c, res)) return rc;
  const u64 slot = subwalk_slot_bytes(S, halo), rows_cap = subwalk_rows_cap(S), runs_cap = subwalk_runs_cap(S);
  u64 ends_b = 0, line_b = 0;  // a call's workspace, sized for the longest window so that no call grows it
  subset_slab_ws_parts(S + halo, &ends_b, &line_b);
  if (int rc = exact_workspace(c, {{&c->d_slot[0], slot}, {&c->d_slot[1], slot}, {&c->d_spar, 16 * W}, {&c->d_rows, rows_cap},
                                   {&c->d_sruns, carry_b + 16 * runs_cap}, {&c->d_sends, ends_b}, {&c->d_sub, line_b}}, res))
    return rc;
  SubCarry *carry = c->d_sruns.as<SubCarry>();
  u64 *d_runs = (u64 *)(c->d_sruns + carry_b);
  HIPCHK(hipMemsetAsync(carry, 0, carry_b, s), "carry");
  TwoSlots w(c, ids_fd, 0, n, res);
  HIPCHK(w.events.create(), "event");
  SubCursor cur;
  SubWindow win = subwalk_window_at(0, W, parent_count);
  int rc = sub_load_window(c, parent_fd, win, res);
  st.windows = 1;
  st.parent_bytes = 16 * win.rows;
  int i = 0;
  ColSlabPos p = colwalk_slab_at(0, S, halo, n);
  if (!rc) rc = stage_col(w, 0, p);
  st.ids_bytes = p.end;
  shockidx_subset_slab_result r2;
  memset(&r2, 0, sizeof r2);
  while (!rc) {
    bool more = !p.last, moved = false;
    ColSlabPos q = p;
    if (more) {  // the slab expected next, on its way while this one runs
      q = colwalk_slab_at(p.lo + p.n, S, halo, n);
      if ((rc = stage_col(w, i ^ 1, q))) break;
      st.ids_bytes += q.end + q.front;
    }
    if ((rc = w.wait(i))) break;
    st.slabs++;
    for (;;) {
      shockidx_slab sl;
      memset(&sl, 0, sizeof sl);
      sl.d_data = c->d_slot[i] + COLWALK_FRONT;
      sl.n = p.n; sl.end = p.end; sl.front = p.front; sl.base = p.lo;
      sl.is_first = p.first; sl.is_last = p.last;
      rc = shockidx_subset_slab_device(c, &sl, n, c->d_spar, win.row0, win.rows, parent_count, ilength, want_runs, carry,
                                       c->d_rows, rows_cap, d_runs, runs_cap, &r2);
      st.calls++;
      res->kernel_ms += r2.kernel_ms;
      if (rc != SHOCKIDX_OK && rc != SHOCKIDX_EFORMAT) {
        if (rc == SHOCKIDX_ESPACE) rc = set_msg(res, SHOCKIDX_EINTERNAL, "internal error: a slab's tables are short");
        else forward_error(res, r2, rc);
        break;
      }
      const int rc_call = rc;
      if ((rc = drain_rows(c, c->d_rows, r2.rows, cur.take_rows(r2.rows), *sinks.rows, nullptr, nullptr, res))) break;
      if (want_runs && (rc = drain_rows(c, d_runs, r2.runs, cur.take_runs(r2.runs), *sinks.runs, nullptr, nullptr, res))) break;
      if (rc_call == SHOCKIDX_EFORMAT) { rc = forward_error(res, r2, SHOCKIDX_EFORMAT); break; }
      if (r2.stop == 2) {  // the same slab against the window that starts at the id's row
        win = subwalk_next_window(r2.next_id, W, parent_count);
        if ((rc = sub_load_window(c, parent_fd, win, res))) break;
        st.windows++;
        st.parent_bytes += 16 * win.rows;
        continue;
      }
      if (r2.stop == 1) {
        if (subwalk_on_open_line(p.lo, r2.next_off) == SubRetry::NoMem) {
          rc = set_msg(res, SHOCKIDX_ENOMEM, "device memory: an id line is longer than a slab slot can hold");
          break;
        }
        q = colwalk_slab_at(r2.next_off, S, halo, n);
        more = moved = true;
      }
      break;
    }
    if (rc || !more) break;
    if (moved) {  // a fresh slot from the open line on
      if ((rc = stage_col(w, i ^ 1, q))) break;
      st.ids_bytes += q.end + q.front;
    }
    p = q;
    i ^= 1;
  }
  rc = w.finish(rc);
  st.held_bytes = workspace_bytes(c);
  if (rc == SHOCKIDX_OK || rc == SHOCKIDX_EFORMAT) {
    res->count = r2.count;
    res->runs = r2.nruns;
    res->size = r2.size;
  }
  res->total_ms = now_ms() - t0;
  return rc;
}

// ---- the chunkrecord index's walk --------------------------------------------------------------
// chunkRecord.Create (chunkrecord.go:41-99) slab by slab through two slots: slot k holds file bytes
// [max(0, k S - H), min(n, (k + 1) S)) from its first byte on, slab k + 1 is copied on the copy
// stream while slab k is walked, each slab's rows go to the sink as they are made, and the loop's
// state travels in the device carry.  sidx_chunkwalk.hpp holds the layout, the sizing and the reason
// no slab is ever submitted twice.  The device holds the two slots, the carry, one slab's
// workspace (c->d_cra, c->d_crb and, for FASTQ, the tile block of the view's record index) and one
// slab's rows.
int chunk_fd_walk(shockidx_ctx *c, int fd, u64 n, int fmt, u64 chunk, u64 S, RowSink &sink, shockidx_result *res) {
  const double t0 = now_ms();
  res->path = 6;
  hipStream_t s = c->stream;
  if (!S) {
    const u64 top = n < CHUNKWALK_MAX_SLAB ? n : CHUNKWALK_MAX_SLAB;
    S = chunkwalk_slab_bytes(dev_budget(c), chunk, chunk_walk_dev(c, top + CHUNKWALK_HALO));
    if (!S) return set_msg(res, SHOCKIDX_ENOMEM, "device memory: the chunkrecord walk needs at least 32 MiB of its budget");
  }
  if (S > n) S = n ? n : 1;
  const u64 vmax = S + CHUNKWALK_HALO;
  const ChunkWalkDev dv = chunk_walk_dev(c, vmax);
  if (int rc = walk_prereqs(c, res)) return rc;
  const u64 slot = chunkwalk_slot_bytes(S), cra = chunkwalk_cra_bytes(vmax, dv.scan_bytes, dv.gslot),
            crb = chunkwalk_crb_bytes(vmax, chunk), row_cap = chunkwalk_row_bound(vmax, chunk);
  if (int rc = exact_workspace(c, {{&c->d_slot[0], slot}, {&c->d_slot[1], slot}, {&c->d_cra, cra}, {&c->d_crb, crb},
                                   {&c->d_crc, dv.carry_bytes}, {&c->d_rows, row_cap}}, res))
    return rc;
  ChunkCarry *carry = c->d_crc.as<ChunkCarry>();
  TwoSlots w(c, fd, 0, n, res);
  HIPCHK(w.events.create(), "event");
  auto stage = [&](u64 k) {  // slab k's slot bytes (empty for an empty file) into slot k mod 2
    const ChunkSlot p = chunkwalk_slot(k, S, n);
    return w.stage(k & 1, 0, p.lo, p.hi);
  };
  const u64 K = chunkwalk_slots(S, n);
  ColRowCursor cur;
  u64 next = 0;
  double t_d2h = 0;
  int kfmt = 0;
  int rc = stage(0);
  for (u64 k = 0; !rc && k < K; ++k) {
    if (k + 1 < K && (rc = stage(k + 1))) break;  // the next slab, on its way while this one is walked
    if ((rc = w.wait(k & 1))) break;
    const ChunkSlot p = chunkwalk_slot(k, S, n);
    const ChunkView v{c->d_slot[k & 1], p.lo, p.hi, n, p.last};
    if (k == 0) {  // the first slab resolves the format (S >= 64 KiB: it holds the bytes detection reads)
      if ((rc = resolve_format(c, v.d, v.hi, SHOCKIDX_RECORD, fmt, s, &kfmt, res))) break;
      res->format = kfmt;
      if (kfmt == SHOCKIDX_FMT_SAM) {
        rc = set_msg(res, SHOCKIDX_EFORMAT, "chunkrecord: sam.SeekChunk never advances (reference loops forever)");
        break;
      }
      if (kfmt != SHOCKIDX_FMT_FASTA && kfmt != SHOCKIDX_FMT_FASTQ) { rc = set_msg(res, SHOCKIDX_EINVAL, "invalid format"); break; }
    }
    shockidx_result r2;
    reset_result(&r2);
    rc = chunk_slab_run(c, v, chunk, k == 0, kfmt, carry, c->d_rows, row_cap, s, &r2);
    res->kernel_ms += r2.kernel_ms;
    res->reruns += r2.reruns;
    if (rc == SHOCKIDX_ESPACE) rc = set_msg(res, SHOCKIDX_EINTERNAL, "internal error: a slab's rows exceed their bound");
    else if (rc) forward_error(res, r2, rc);
    if (rc) break;
    rc = col_rows_to_sink(c, r2.count, cur, &next, sink, &t_d2h, res);
  }
  if ((rc = w.finish(rc))) {
    res->count = 0;
    return rc;
  }
  if (next != n) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_END_MSG);
  finish_walk(res, kfmt, cur.total, 6, res->kernel_ms, res->kernel_ms, t_d2h, t0);
  res->status = SHOCKIDX_OK;
  return SHOCKIDX_OK;
}

// ---- the download filters' walk ----------------------------------------------------------------
// GET /node/{id}?download&filter=F (controller/node/single.go:490-526; its seek / length form
// :194-257) over a FASTQ section of a file: the section slab by slab through the two slots (slab
// k + 1 copied on the copy stream while slab k runs), the reader's position and the filter's counter
// in the device carry, each slab's output through the pinned buffer to out_fd in order -- what
// io.Copy writes to the response (request/streamer.go:91-96), the bytes before a reader error
// included.  sidx_filtwalk.hpp holds the sizing and the restart rule.  The device holds the two
// slots, the view, the carry with one slab's output, one slab's workspace (c->d_sub, the tile block
// of the view's record index) and one slab's rows, all sized up front.
namespace {

// every byte of [p, p + k) to fd.  SIGPIPE is blocked around the writes, and one raised by them is
// taken off the thread, so a reader that closed its end is EPIPE in the result whatever the
// process does with the signal.
int write_all(int fd, const uint8_t *p, size_t k, Err res) {
  sigset_t pipe_set, old, pend;
  sigemptyset(&pipe_set);
  sigaddset(&pipe_set, SIGPIPE);
  (void)pthread_sigmask(SIG_BLOCK, &pipe_set, &old);
  (void)sigpending(&pend);
  const bool was_pending = sigismember(&pend, SIGPIPE) == 1;
  int err = 0;
  while (k) {
    const ssize_t r = write(fd, p, k);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) {
      err = r < 0 ? errno : EIO;
      break;
    }
    p += r;
    k -= (size_t)r;
  }
  if (err == EPIPE && !was_pending) {
    const struct timespec zero = {0, 0};
    while (sigtimedwait(&pipe_set, nullptr, &zero) < 0 && errno == EINTR) {}
  }
  (void)pthread_sigmask(SIG_SETMASK, &old, nullptr);
  return err ? set_msg(res, SHOCKIDX_EIO, std::string("write: ") + strerror(err)) : 0;
}

void filter_stats_end(shockidx_ctx *c, shockidx_subset_result *res, double t_d2h, double t_write, double t0) {
  shockidx_filter_stats &st = c->filter_stats;
  st.peak_bytes = workspace_bytes(c);
  st.kernel_us = (u64)(res->kernel_ms * 1000.0);
  st.d2h_us = (u64)(t_d2h * 1000.0);
  st.write_us = (u64)(t_write * 1000.0);
  res->gather_ms = t_d2h + t_write;
  res->total_ms = now_ms() - t0;
}

// The whole path: the section resident, filter_section over it, the output written.
int filter_fd_whole(shockidx_ctx *c, int kind, int fd, u64 off, u64 n, int out_fd, bool fastq, shockidx_subset_result *res) {
  const double t0 = now_ms();
  c->filter_stats.path = 1;
  double t_d2h = 0, t_write = 0;
  auto run = [&]() -> int {
    if (int rc = walk_prereqs(c, res)) return rc;
    shockidx_result r0;
    reset_result(&r0);
    if (int rc = stage_fd(c, fd, off, n, c->stream, &r0)) return forward_error(res, r0, rc);
    // FASTQ: the worst case (no retry); FASTA / SAM: twice the section first, the exact size on ESPACE
    u64 cap = fastq ? filtwalk_out_bound(n, filtwalk_rows_cap(n), filtwalk_rows_cap(n)) : 2 * n;
    int rc = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      if ((rc = c->d_fout.ensure(cap + FILTWALK_PAD, res))) return rc;
      reset_result(res);
      rc = filter_section(c, kind, c->d_in, n, c->d_fout, cap, res, false);
      if (rc != SHOCKIDX_ESPACE) break;
      cap = res->size;
    }
    if (rc != SHOCKIDX_OK && rc != SHOCKIDX_EFORMAT) return rc;
    // (a failed drain replaces the reader's error: the stream did not reach the caller)
    if (int rc2 = drain_bytes(c, c->d_fout, res->size, out_fd, &t_d2h, &t_write, res)) return rc2;
    return rc;
  };
  const int rc = run();
  filter_stats_end(c, res, t_d2h, t_write, t0);
  return rc;
}

}  // namespace

int drain_bytes(shockidx_ctx *c, const uint8_t *d_src, u64 total, int out_fd, double *t_d2h, double *t_write, Err res) {
  for (u64 done = 0; done < total;) {
    const u64 k = total - done < STAGE_BYTES ? total - done : STAGE_BYTES;
    const double ta = now_ms();
    HIPCHK(hipMemcpyAsync(c->h_rows[0], d_src + done, k, hipMemcpyDeviceToHost, c->stream), "output copy");
    HIPCHK(hipStreamSynchronize(c->stream), "output copy");
    const double tb = now_ms();
    if (int rc = write_all(out_fd, c->h_rows[0], k, res)) return rc;
    if (t_d2h) *t_d2h += tb - ta;
    if (t_write) *t_write += now_ms() - tb;
    done += k;
  }
  return 0;
}

int filter_fd_walk(shockidx_ctx *c, int kind, const char *filter, int fd, u64 off, u64 n, int out_fd, u64 S, u64 halo,
                   shockidx_subset_result *res) {
  const double t0 = now_ms();
  shockidx_filter_stats &st = c->filter_stats;
  memset(&st, 0, sizeof st);
  st.path = 2;
  (void)kind;
  const u64 budget = dev_budget(c);
  if (!halo) halo = filtwalk_default_halo(budget);
  const u64 top = n < FILTWALK_MAX_SLAB ? n : FILTWALK_MAX_SLAB;
  const FiltWalkDev dv = filter_walk_dev(c, top + halo);
  if (!S) {
    S = filtwalk_slab_bytes(budget, halo, n, dv);
    if (!S) return set_msg(res, SHOCKIDX_ENOMEM, "device memory: the filter walk needs at least 32 MiB of its budget");
  }
  if (S > n) S = n > FILTWALK_DETECT ? n : FILTWALK_DETECT;
  if (halo > S) halo = S;  // (the position a slab carries out lies within the next slab's owned bytes)
  st.slab_bytes = S;
  st.halo_bytes = halo;
  double t_d2h = 0, t_write = 0;
  auto run = [&]() -> int {
    if (int rc = walk_prereqs(c, res)) return rc;
    const FiltWalkPlan plan = filtwalk_plan(S, halo, n, dv);
    if (int rc = exact_workspace(c, {{&c->d_slot[0], plan.slot}, {&c->d_slot[1], plan.slot}, {&c->d_fview, plan.view},
                                     {&c->d_rows, plan.rows}, {&c->d_sub, plan.ws}, {&c->d_fout, dv.carry_bytes + plan.out}}, res))
      return rc;
    FiltCarry *carry = c->d_fout.as<FiltCarry>();
    uint8_t *d_out = c->d_fout + dv.carry_bytes;
    TwoSlots w(c, fd, off, n, res);
    HIPCHK(w.events.create(), "event");
    auto stage = [&](int i, const FiltSlabPos &p) { return w.stage(i, 0, p.lo, p.lo + p.end); };
    int i = 0;
    FiltSlabPos p = filtwalk_slab_at(0, S, halo, n, true);
    int rc = stage(0, p);
    while (!rc) {
      FiltSlabPos q = p;
      if (!p.last) {  // the slab expected next, on its way while this one runs
        q = filtwalk_slab_at(p.lo + p.n, S, halo, n, false);
        if ((rc = stage(i ^ 1, q))) break;
      }
      if ((rc = w.wait(i))) break;
      st.slabs++;
      shockidx_slab sl;
      memset(&sl, 0, sizeof sl);
      sl.d_data = c->d_slot[i].get();
      sl.n = p.n; sl.end = p.end; sl.front = 0; sl.base = p.lo;
      sl.is_first = p.first; sl.is_last = p.last;
      shockidx_subset_result r2;
      uint64_t pos = 0;
      rc = shockidx_filter_slab_device(c, filter, &sl, n, carry, d_out, plan.out, &pos, &r2);
      res->kernel_ms += r2.kernel_ms;
      if (rc != SHOCKIDX_OK && rc != SHOCKIDX_EFORMAT) {
        if (rc == SHOCKIDX_ESPACE) rc = set_msg(res, SHOCKIDX_EINTERNAL, "internal error: a slab's output exceeds its bound");
        else forward_error(res, r2, rc);
        break;
      }
      const int rc_call = rc;
      if ((rc = drain_bytes(c, d_out, r2.size, out_fd, &t_d2h, &t_write, res))) break;
      res->count += r2.count;
      res->size += r2.size;
      if (rc_call == SHOCKIDX_EFORMAT) { rc = forward_error(res, r2, SHOCKIDX_EFORMAT); break; }
      if (p.last) break;
      const FiltNext next = filtwalk_next(p.lo, q.lo, pos);
      if (next == FiltNext::NoMem) {
        rc = set_msg(res, SHOCKIDX_ENOMEM, "device memory: a record is longer than a slab slot can hold");
        break;
      }
      if (next == FiltNext::Restart) {  // a fresh slot from the open record on
        q = filtwalk_slab_at(pos, S, halo, n, false);
        st.restarts++;
        if ((rc = stage(i ^ 1, q))) break;
      }
      p = q;
      i ^= 1;
    }
    return w.finish(rc);
  };
  const int rc = run();
  filter_stats_end(c, res, t_d2h, t_write, t0);
  return rc;
}

int filter_fd_any(shockidx_ctx *c, int kind, const char *filter, int fd, u64 off, u64 n, int out_fd,
                  shockidx_subset_result *res) {
  memset(&c->filter_stats, 0, sizeof c->filter_stats);
  c->filter_stats.path = 1;
  int kfmt = SHOCKIDX_FMT_FASTQ;  // fq2fa reads everything as FASTQ
  if (kind == 2) {  // anonymize: DetermineFormat over the section's first 32 KiB (multi.go:43-62)
    if (!n) return set_msg(res, SHOCKIDX_EFORMAT, "Invalid file type for filter");  // errors.go:20
    const u64 m = n < FILTWALK_DETECT ? n : FILTWALK_DETECT;
    shockidx_result r0;
    reset_result(&r0);
    if (int rc = stage_fd(c, fd, off, m, c->stream, &r0)) return forward_error(res, r0, rc);
    if (int rc = resolve_format(c, c->d_in, m, SHOCKIDX_RECORD, SHOCKIDX_FMT_AUTO, c->stream, &kfmt, res)) return rc;
  }
  if (!n) return SHOCKIDX_OK;  // fq2fa over an empty section delivers nothing
  const u64 budget = dev_budget(c);
  const FiltWalkDev dv = filter_walk_dev(c, n);
  if (kfmt == SHOCKIDX_FMT_FASTQ) {
    if (filtwalk_whole_bytes(n, dv) <= budget) return filter_fd_whole(c, kind, fd, off, n, out_fd, true, res);
    return filter_fd_walk(c, kind, filter, fd, off, n, out_fd, 0, 0, res);
  }
  if (filtwalk_whole_other_bytes(n, dv) <= budget) return filter_fd_whole(c, kind, fd, off, n, out_fd, false, res);
  return set_msg(res, SHOCKIDX_ENOMEM,
                 kfmt == SHOCKIDX_FMT_FASTA ? "device memory: the FASTA section does not fit the budget (only FASTQ sections are filtered in slabs)"
                                            : "device memory: the SAM section does not fit the budget (only FASTQ sections are filtered in slabs)");
}

}  // namespace sidx_host
