// sidx_pipeline.cpp -- the slab pipelines: builds that index a node slab by slab while the rest
// of it is still crossing PCIe (sidx_slabwalk.hpp holds their arithmetic and decisions).
//
// Slab-pipelined build over a file descriptor -- the drop-in path: node.AsyncIndexer opens the
// node file and hands it to Create (node/index.go:107-121).  The file is DMA'd to HBM on the copy
// stream (out of the page cache, or through the pinned staging buffers); an index thread runs
// each slab as soon as its bytes and a 4 MiB halo have arrived, with the previous slab's exact end
// state as its incoming state (the multi-GPU slab kernels, no guess), and hands the slab's rows to
// the sink while later slabs are still being read -- so after the last byte crosses PCIe only the
// last slab's index and rows are left.  FASTQ, FASTA and line.
//
// Two layouts in HBM (round 6):
//  - whole: the node in one buffer (n bytes), 1 GiB slabs -- when one_pass_bytes(n) fits the
//    device budget, so the rare fallback below can index the node in place;
//  - ring: two slot buffers of S + 64 KiB + 4 MiB (slab k goes to slot k mod 2 with the 64 KiB
//    before it and its halo; the halo and front bytes cross PCIe twice, 0.4 %), S sized to the
//    budget -- so the device footprint does not grow with the node, like record.go's 4 KiB
//    bufio.Reader (record.go:51-83, fastq.go:136).  The producer reuses a slot once the index
//    thread is done with the slab in it.
// Anything but a clean slab (a format error, a record past the halo, a device flag, SAM, no
// detectable format) ends the slab walk.  Whole layout: the one-pass build of the whole file,
// which is in HBM by then (*fell_back = true, nothing reported to the caller).  Ring layout: the
// rows of the clean slabs before it are final (exact incoming states), and the rest of the file,
// from the start r of the first record not yet emitted, is re-read and indexed in one pass as a
// node of its own -- a record boundary resets every reader (FASTQ's skip loop and `empty`,
// FASTA's piece after UnreadByte, a line), so its rows are the file's rows shifted by r; its
// count and error complete the table.  The rest is walked through the same slots again, its
// first slab starting at r (*restart = r: build_fd_pipelined below loops), so a record longer than
// the halo but not than a slab costs one re-read of that record; only a record the walk cannot
// close from its own start (longer than a slab) takes the one-pass build of the rest, which needs
// one_pass_bytes of it within the budget, or the build fails with SHOCKIDX_ENOMEM.
// base > 0: this walk is such a rest -- the file bytes [base, base + n) as a node of its own
// (rows at absolute file offsets, numbered from row0; always the ring layout).
// *done = false: not applicable (small file, other kind), nothing was read.
//
// The host-memory pipeline (build_host_pipelined, FASTQ bodies in pinned memory) is the same walk
// over the whole layout without a second thread: the copies are all issued up front.
//
// The walks that carry their state on the device (column, subset, chunkrecord) are in
// sidx_walks.cpp; sidx_walk.hpp has what they share with these.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_slabwalk.hpp"
#include "sidx_launch.hpp"
#include "sidx_walk.hpp"

using namespace sidx;

namespace sidx_host {

// ---- row sinks -------------------------------------------------------------------------------
// sized up front for the file (16 bytes per 32 input bytes: only the pages the rows touch are
// ever faulted in), so the usual table is never copied while it grows
TableSink::TableSink(u64 n) {
  cap = (size_t)(n / 32 + 4096) * 16;
  out = (uint8_t *)alloc_rows_out(cap);
  if (!out) cap = 0;
}
TableSink::~TableSink() { free(out); }
int TableSink::put(const uint8_t *src, u64 first, u64 nrows, Err res) {
  const size_t need = (size_t)(first + nrows) * 16;
  if (need > cap) {
    size_t nc = cap ? cap : (64u << 20);
    while (nc < need) nc *= 2;
    uint8_t *o2 = (uint8_t *)alloc_rows_out(nc);
    if (!o2) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
    if (out) memcpy(o2, out, (size_t)first * 16);
    free(out);
    out = o2;
    cap = nc;
  }
  memcpy(out + (size_t)first * 16, src, (size_t)nrows * 16);
  return 0;
}
int FileSink::put(const uint8_t *src, u64 first, u64 nrows, Err res) {
  size_t left = (size_t)nrows * 16;
  off_t at = (off_t)(first * 16);
  while (left) {
    const ssize_t w = pwrite(fd, src, left > (1u << 30) ? (1u << 30) : left, at);
    if (w < 0) {
      if (errno == EINTR) continue;
      return set_msg(res, SHOCKIDX_EIO, strerror(errno));
    }
    src += w;
    at += w;
    left -= (size_t)w;
  }
  return 0;
}

namespace {

// Slab k of the layout, at d_slab, indexed into the context's rows from row `row_off` on (room
// for row_cap rows) with the previous slab's end state.  grow: a slab with more rows than its
// share (records or lines under 32 bytes on average) is indexed again into rows grown to its
// count, while its bytes are still in place.  *row_base: the rows before it are not the slab's
// (the record open at a later slab's start is the previous slab's).
int index_slab(shockidx_ctx *c, const SlabLayout &lay, u64 k, const uint8_t *d_slab, int kfmt, u64 base, u64 state,
               u64 row_off, u64 row_cap, bool grow, DevResult *dr, shockidx_result *r2, u64 *row_base) {
  SlabGeom g;
  g.n = lay.len(k);
  g.end = lay.end(k);
  g.front = lay.front(k);
  g.base = base + lay.lo(k);  // (rows and FASTA error pieces at file offsets)
  g.state_in = kfmt == F_FASTQ ? (state & 3) : kfmt == F_FASTA ? (state & 1) : 0;
  g.row_base = *row_base = k ? 1 : 0;
  g.eof = lay.eof(k);
  g.file_start = k == 0;
  g.d_summary = c->d_small + SMALL_SLABSUM;
  int rc = run_index(c, d_slab, g.n, kfmt, c->d_rows + 2 * row_off, row_cap, c->stream, dr, r2, &g);
  if (grow && rc == 0 && dr->flags == RF_CAPACITY && dr->count > g.row_base &&
      c->d_rows.ensure(dr->count - g.row_base + 4096, r2) == 0)
    rc = run_index(c, d_slab, g.n, kfmt, c->d_rows, c->d_rows.cap, c->stream, dr, r2, &g);
  return rc;
}

// ---- the fd walk -----------------------------------------------------------------------------
// How the index thread's walk over the slabs ended.  A library error code (< 0) travels beside
// it, in WalkResult::err.
enum class WalkEnd {
  Clean,     // every slab was clean
  FallBack,  // a slab ended the walk (or the producer failed): whole layout the one-pass build,
             //   ring a restart at the first record not yet emitted or the one-pass build of the rest
  NoFormat,  // no detectable format (multi.go:43-62 reads the first 32 KiB only): reported as is
  GoError,   // ring: a Go format error in a slab (err_dr); the rows before it are in the sink
  Error,     // err, message in cres
};
struct WalkResult {
  WalkEnd end = WalkEnd::Clean;
  int err = 0;
  DevResult err_dr{};
  shockidx_result cres;  // the index thread's messages and kernel times
  RowCursor cur;
  int kfmt = 0;
  double t_d2h = 0;
  void fail(int code) {
    end = WalkEnd::Error;
    err = code;
  }
};

// What the producer (the calling thread) and the index thread tell each other, slab by slab.
class SlabHandoff {
 public:
  // producer: slab k's arrival event is recorded on the copy stream
  void publish(u64 k) { set([&] { recorded = k + 1; }); }
  // producer: it gave up (the index thread falls back once it has run out of slabs)
  void fail() { set([&] { prod_failed = true; }); }
  // index thread: until slab k is published; false: the producer failed before it
  bool wait_arrived(u64 k) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return recorded > k || prod_failed; });
    return recorded > k;
  }
  // index thread: done with slab k (its slot may be refilled)
  void release(u64 k) { set([&] { freed = k + 1; }); }
  // producer (ring): until slot k mod 2 is free, i.e. the index thread is done with slab k - 2;
  // false: the index thread ended before that
  bool wait_slot(u64 k) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return freed + 2 > k || ix_over; });
    return freed + 2 > k;
  }
  // marks the index side over, whatever way its thread ends (wakes the producer)
  struct IndexSide {
    SlabHandoff &h;
    ~IndexSide() { h.set([&] { h.ix_over = true; }); }
  };

 private:
  template <class F> void set(F f) {
    {
      std::lock_guard<std::mutex> g(mu);
      f();
    }
    cv.notify_all();
  }
  std::mutex mu;
  std::condition_variable cv;
  u64 recorded = 0;  // slabs whose arrival event is recorded on the copy stream
  u64 freed = 0;     // slabs the index thread is done with
  bool prod_failed = false, ix_over = false;
};

// One walk's fixed inputs and the state its two threads share.
struct Walk {
  shockidx_ctx *c;
  int fd, kind, fmt;
  u64 base;  // the walk's node is file bytes [base, base + lay.n)
  SlabLayout lay;
  RowSink &sink;
  SlabEvents &events;
  SlabHandoff hand;
  // where slab k's first byte is (ring: after the front bytes in its slot)
  uint8_t *slab_ptr(u64 k) const { return lay.ring ? c->d_slot[k & 1] + lay.front(k) : c->d_in + lay.lo(k); }
};

// The table's next m rows (device rows [0, m), `shift` added to their offsets) into the sink.
// They continue the table (record.go:51-83): the first starts where the last row before them
// ended.  0, or the library code (message in res).
int rows_to_sink(Walk &w, WalkResult &o, u64 m, u64 shift, Err res) {
  auto accept = [&](u64 *rows, u64 k, u64 done) {
    for (u64 i = 0; shift && i < k; ++i) rows[2 * i] += shift;
    return o.cur.accept(rows, k, done == 0) ? 0 : set_msg(res, SHOCKIDX_EINTERNAL, SLAB_SEAM_MSG);
  };
  return drain_rows(w.c, w.c->d_rows, m, o.cur.total, w.sink, accept, &o.t_d2h, res);
}

// The index thread: slab k after its bytes (+ halo) have arrived.
void index_slabs(Walk &w, WalkResult &o) {
  SlabHandoff::IndexSide over{w.hand};
  shockidx_ctx *c = w.c;
  hipStream_t s = c->stream;
  const SlabLayout &lay = w.lay;
  if (hipSetDevice(c->device) != hipSuccess) return o.fail(set_msg(&o.cres, SHOCKIDX_EHIP, "hipSetDevice"));
  u64 state = 0;
  for (u64 k = 0; k < lay.count(); ++k) {
    if (!w.hand.wait_arrived(k)) { o.end = WalkEnd::FallBack; return; }
    if (hipStreamWaitEvent(s, w.events.ev[k], 0) != hipSuccess) return o.fail(set_msg(&o.cres, SHOCKIDX_EHIP, "wait slab"));
    if (k == 0) {
      int rc = resolve_format(c, w.slab_ptr(0), lay.ring ? lay.end(0) : lay.n, w.kind, w.fmt, s, &o.kfmt, &o.cres);
      if (rc < 0) return o.fail(rc);
      if (rc) { o.end = WalkEnd::NoFormat; return; }
      if (o.kfmt != F_FASTQ && o.kfmt != F_FASTA && o.kfmt != F_LINE) { o.end = WalkEnd::FallBack; return; }
    }
    DevResult dr;
    shockidx_result r2;
    reset_result(&r2);
    u64 row_base = 0;
    const int rc = index_slab(c, lay, k, w.slab_ptr(k), o.kfmt, w.base, state, 0, c->d_rows.cap, true, &dr, &r2, &row_base);
    w.hand.release(k);  // (run_index waited for its kernels: the slot's bytes are no longer read)
    if (rc < 0) return o.fail(forward_error(&o.cres, r2, rc));
    o.cres.kernel_ms += r2.kernel_ms;
    o.cres.index_ms += r2.index_ms;
    const SlabOutcome oc = classify(rc, dr, row_base, lay.last(k), lay.ring);
    if (oc == SlabOutcome::FallBack) { o.end = WalkEnd::FallBack; return; }
    if (int e = rows_to_sink(w, o, dr.count - row_base, 0, &o.cres)) return o.fail(e);
    state = dr.state_out;
    if (oc == SlabOutcome::GoError) {
      o.err_dr = dr;
      o.end = WalkEnd::GoError;
      return;
    }
    if (oc == SlabOutcome::Partial) { o.end = WalkEnd::FallBack; return; }
  }
}

// The producer: the node's bytes onto the copy stream, each slab published once its bytes (and
// halo) are all issued.  Ring: slab by slab into the slots; whole: 256 MiB at a time.
int produce(Walk &w, PageCacheSource &src, Err res) {
  shockidx_ctx *c = w.c;
  const SlabLayout &lay = w.lay;
  const u64 K = lay.count();
  auto publish = [&](u64 k) -> int {
    if (hipError_t e = hipEventRecord(w.events.ev[k], c->s_copy)) return set_hip(res, e, "event");
    w.hand.publish(k);
    return 0;
  };
  int prc = 0;
  if (lay.ring) {
    for (u64 k = 0; k < K && !prc; ++k) {
      if (!w.hand.wait_slot(k)) break;  // the index thread ended (fallback or error)
      const u64 lo = lay.lo(k), fk = lay.front(k);
      prc = src.copy_range(c->d_slot[k & 1], lo - fk, lo + lay.end(k), lo - fk);
      if (!prc) prc = publish(k);
    }
  } else {
    constexpr u64 CH = 256ull << 20;
    u64 off = 0, ks = 0;
    while (off < lay.n && !prc) {
      const u64 e = off + CH < lay.n ? off + CH : lay.n;
      prc = src.copy_range(c->d_in + off, off, e, 0);
      off = e;
      while (!prc && ks < K && lay.lo(ks) + lay.end(ks) <= off) prc = publish(ks++);
    }
  }
  return prc;
}

// Both threads of a walk, until the index thread has ended and every copy has landed.  Returns
// the producer's code; the walk's outcome is in o.
int transfer(Walk &w, WalkResult &o, Err res) {
  PageCacheSource src(w.c, w.fd, w.base, w.lay.n, res);
  std::thread ix(index_slabs, std::ref(w), std::ref(o));
  int prc = produce(w, src, res);
  if (prc) w.hand.fail();
  ix.join();
  const hipError_t se = src.drain();  // before the pages are unpinned and unmapped (~PageCacheSource)
  if (se != hipSuccess && !prc) prc = set_hip(res, se, "H2D sync");
  return prc;
}

// the record walk ends here: its count and the times its index thread carried
void finish_record_walk(shockidx_result *res, int kfmt, u32 path, const WalkResult &o, double t0) {
  finish_walk(res, kfmt, o.cur.total, path, o.cres.kernel_ms, o.cres.index_ms, o.t_d2h, t0);
}

// Ring, no progress (a record the walk cannot close from its own start): the rest of the file
// from the first record not yet emitted, as a node of its own, in one pass; its rows, shifted
// by r, continue the table.
int one_pass_rest(Walk &w, WalkResult &o, shockidx_result *res, double t0) {
  shockidx_ctx *c = w.c;
  hipStream_t s = c->stream;
  const u64 r = o.cur.next_off, end = w.base + w.lay.n;
  for (auto &slot : c->d_slot) slot.drop();
  if (one_pass_bytes(end - r) > dev_budget(c))
    return set_msg(res, SHOCKIDX_ENOMEM, "device memory: the node's one-pass fallback does not fit the device budget");
  shockidx_result r3;
  reset_result(&r3);
  if (int rc = stage_fd(c, w.fd, r, end - r, s, &r3)) return forward_error(res, r3, rc);
  const int sfmt = o.cur.total ? (o.kfmt == F_LINE ? SHOCKIDX_FMT_AUTO : o.kfmt) : w.fmt;
  const int rc = build_resident(c, c->d_in, end - r, w.kind, sfmt, s, &r3);
  if (rc < 0) return forward_error(res, r3, rc);
  if (int e = rows_to_sink(w, o, r3.count, r, res)) return e;
  o.cres.kernel_ms += r3.kernel_ms;
  o.cres.index_ms += r3.index_ms;
  finish_record_walk(res, r3.format, 4, o, t0);
  forward_error(res, r3, r3.status);
  res->reruns = r3.reruns + 1;
  return rc;
}

// A Go error in a slab: the rows before it are in the sink; its text as the one-pass build
// reports it.  The FASTA piece is read back from the file (it may begin before the slot holding
// the slab).
int finish_go_error(Walk &w, WalkResult &o, shockidx_result *res, double t0) {
  finish_record_walk(res, o.kfmt, 4, o, t0);
  res->term_code = o.err_dr.code;
  if (o.err_dr.code == ST_FA_INVALID)
    return fasta_error_text(res, o.err_dr.err_len, [&](char *dst, u64 k) -> int {
      return pread(w.fd, dst, (size_t)k, (off_t)o.err_dr.err_pos) == (ssize_t)k ? 0 : set_msg(res, SHOCKIDX_EIO, "error text read");
    });
  const char *m = status_message(o.err_dr.code);
  if (!m) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: unknown device status");
  return set_msg(res, SHOCKIDX_EFORMAT, m);
}

// The walk's device buffers: the two slots (ring) or the whole node (c->d_in), the per-slab rows
// and the pinned row staging.  The caches of the other layout go first.
int prepare_buffers(shockidx_ctx *c, const SlabLayout &lay, shockidx_result *res) {
  hipStream_t s = c->stream;
  if (int rc = walk_prereqs(c, res)) return rc;
  const u64 SLOT = RING_FRONT + lay.S + PIPE_HALO + 64;  // (kept by the context, like its other caches, until a trim)
  if (lay.ring) {
    // slots of another size: the caches of earlier (larger) builds go first (the node buffer of a
    // one-pass build, rows); slots of this size: only the node buffer goes
    if (int rc = exact_workspace(c, {{&c->d_slot[0], SLOT}, {&c->d_slot[1], SLOT}}, res)) return rc;
    if (c->d_in) {
      (void)hipStreamSynchronize(s);
      c->d_in.drop();
    }
  } else {
    if (c->d_slot[0] || c->d_slot[1]) {  // (slots of an earlier build within a cap: not needed by this one)
      (void)hipStreamSynchronize(s);
      for (auto &slot : c->d_slot) slot.drop();
    }
    if (int rc = c->d_in.ensure(lay.n + 64, res)) return rc;
  }
  // per slab its rows' device capacity (reused slab after slab); a slab with more rows (records
  // or lines under 32 bytes on average) overflows it and is indexed again (index_slab)
  return c->d_rows.ensure(lay.S / 32 + 4096, res);
}

// One walk over the file bytes [base, base + n) (the header comment of this file).
int build_fd_walk(shockidx_ctx *c, int fd, u64 n, int kind, int fmt, RowSink &sink, shockidx_result *res,
                  bool *done, bool *fell_back, u64 base, u64 row0, u64 *restart) {
  *done = false;
  *fell_back = false;
  *restart = 0;
  if ((kind != SHOCKIDX_RECORD && kind != SHOCKIDX_LINE) || getenv("SHOCKIDX_NO_FD_PIPE") ||
      (kind == SHOCKIDX_RECORD && fmt != SHOCKIDX_FMT_AUTO && fmt != SHOCKIDX_FMT_FASTQ && fmt != SHOCKIDX_FMT_FASTA))
    return 0;
  const u64 budget = dev_budget(c);
  const bool ring = base || one_pass_bytes(n) > budget || getenv("SHOCKIDX_FD_RING");
  const u64 S = ring ? ring_slab_bytes(budget) : PIPE_SLAB;
  if (!S) return set_msg(res, SHOCKIDX_ENOMEM, "device memory: the build needs at least 256 MiB of its budget");
  if (!ring && n < 2 * S) return 0;  // (whole layout: under 2 GiB the plain staging + one pass is as fast)
  const double t0 = now_ms();
  const SlabLayout lay{n, S, ring};
  if (int rc = prepare_buffers(c, lay, res)) return rc;
  SlabEvents events(lay.count(), c->s_copy);  // (outlives the transfer's copies)
  HIPCHK(events.create(), "event");
  *done = true;
  Walk w{c, fd, kind, fmt, base, lay, sink, events, {}};
  WalkResult o;
  reset_result(&o.cres);
  o.cur = RowCursor{row0, base, 0};
  if (int prc = transfer(w, o, res)) return prc;
  switch (o.end) {
    case WalkEnd::Error:
      return forward_error(res, o.cres, o.err);
    case WalkEnd::NoFormat: {  // the detection's error, as the one-pass build reports it (no rows)
      const int code = o.cres.status ? o.cres.status : SHOCKIDX_EFORMAT;
      forward_error(res, o.cres, code);
      res->count = 0;
      res->total_ms = now_ms() - t0;
      return code;
    }
    case WalkEnd::GoError:
      return finish_go_error(w, o, res, t0);
    case WalkEnd::FallBack:
      if (ring && o.cur.next_off > base) {
        // the rest from r = next_off as a node of its own, through the same slots (the caller loops)
        *restart = o.cur.next_off;
        finish_record_walk(res, o.kfmt, 4, o, t0);
        return 0;
      }
      if (ring) return one_pass_rest(w, o, res, t0);
      // the whole file, one pass (it is all in HBM once the copy stream drained)
      *fell_back = true;
      reset_result(res);
      res->h2d_ms = now_ms() - t0;
      return build_resident(c, c->d_in, n, kind, fmt, c->stream, res);
    case WalkEnd::Clean:
      break;
  }
  // the table ends where the file does (FASTQ: or before trailing blank lines)
  auto byte_at = [&](u64 off, uint8_t *b) { return pread(fd, b, 1, (off_t)off) == 1; };
  if (!table_ends_at_file_end(o.kfmt, o.cur.next_off, base + n, o.cur.last_len, byte_at))
    return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_END_MSG);
  finish_record_walk(res, o.kfmt, ring ? 4 : 3, o, t0);  // the slab pipeline (4: through the two slots)
  res->status = SHOCKIDX_OK;
  return SHOCKIDX_OK;
}

}  // namespace

// The fd build: build_fd_walk over the file, and again over the rest from each restart point
// (a record longer than the halo ended a walk through the slots), rows numbered on.
int build_fd_pipelined(shockidx_ctx *c, int fd, u64 n, int kind, int fmt, RowSink &sink, shockidx_result *res,
                       bool *done, bool *fell_back) {
  const double t0 = now_ms();
  u64 base = 0, row0 = 0;
  int f = fmt;
  double kms = 0, ims = 0, dms = 0;
  uint32_t reruns = 0;
  for (;;) {
    u64 restart = 0;
    const int rc = build_fd_walk(c, fd, n - base, kind, f, sink, res, done, fell_back, base, row0, &restart);
    if (rc || !restart) {
      if (base) {  // the walks before this one
        *done = true;
        res->kernel_ms += kms;
        res->index_ms += ims;
        res->d2h_ms += dms;
        res->reruns += reruns;
        res->path = 4;
        res->total_ms = now_ms() - t0;
        res->h2d_ms = res->total_ms - res->d2h_ms - res->kernel_ms;
      }
      return rc;
    }
    kms += res->kernel_ms;
    ims += res->index_ms;
    dms += res->d2h_ms;
    ++reruns;
    row0 = res->count;
    f = res->format == SHOCKIDX_FMT_LINE ? SHOCKIDX_FMT_AUTO : res->format;  // the format found at the file's start
    base = restart;
  }
}

// Slab-pipelined FASTQ record build of a pinned host body: the body crosses PCIe in 1 GiB
// slabs on a copy stream while the compute stream indexes slab k as soon as its bytes and a
// 4 MiB halo have arrived, with slab k - 1's exact end state as its incoming state (the slab
// kernels of the multi-GPU protocol, with no guess), and the calling thread copies slab k's
// rows out while later slabs are still arriving -- so only the last slab's index and rows
// are left after the H2D.  Anything but a clean slab (an error, a blank group before the end,
// a record past the halo, any device flag) falls back to the one-pass build of the whole body,
// which is in HBM by then.  *done = 0: not applicable (the caller runs the plain path).
int build_host_pipelined(shockidx_ctx *c, const void *data, u64 n, int kind, int fmt, uint64_t **rows,
                         shockidx_result *res, bool *done) {
  *done = false;
  if (kind != SHOCKIDX_RECORD || n < 2 * PIPE_SLAB || !host_pinned(data, n) ||
      (fmt != SHOCKIDX_FMT_AUTO && fmt != SHOCKIDX_FMT_FASTQ) || getenv("SHOCKIDX_NO_HOST_PIPE"))
    return 0;
  const double t0 = now_ms();
  hipStream_t s = c->stream;
  if (int rc = walk_prereqs(c, res, false)) return rc;  // (its rows go straight to the table: no row buffers)
  if (int rc = c->d_in.ensure(n + 64, res)) return rc;
  const SlabLayout lay{n, PIPE_SLAB, false};
  const u64 K = lay.count();
  SlabEvents events(K, c->s_copy);
  std::vector<hipEvent_t> &ev = events.ev;
  for (u64 k = 0; k < K; ++k) {
    HIPCHK(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming), "event");
    HIPCHK(hipMemcpyAsync(c->d_in + lay.lo(k), (const uint8_t *)data + lay.lo(k), lay.len(k), hipMemcpyHostToDevice, c->s_copy), "H2D");
    HIPCHK(hipEventRecord(ev[k], c->s_copy), "event");
  }
  *done = true;
  auto plain = [&]() -> int {  // the whole body, one pass (after every slab has arrived)
    HIPCHK(hipStreamSynchronize(c->s_copy), "H2D sync");
    const double th = now_ms();
    reset_result(res);
    res->h2d_ms = th - t0;
    int rc = build_resident(c, c->d_in, n, kind, fmt, s, res);
    if (rc < 0) return rc;
    if (int rc2 = fetch_rows(c, res->count, s, rows, res)) return rc2;
    res->total_ms = now_ms() - t0;
    return rc;
  };
  HIPCHK(hipStreamWaitEvent(s, ev[0], 0), "wait slab 0");
  int kfmt = 0;
  if (int rc = resolve_format(c, c->d_in, n, kind, fmt, s, &kfmt, res)) {
    if (rc < 0) return rc;
    return plain();  // no format: the plain build reports it
  }
  if (kfmt != SHOCKIDX_FMT_FASTQ) return plain();
  const u64 rcap = n / 32 + 4096;
  if (int rc = c->d_rows.ensure(rcap, res)) return rc;
  size_t out_cap = (size_t)(n / 128 + 4096) * 16;
  struct FreeDel {
    void operator()(uint8_t *p) const { free(p); }
  };
  std::unique_ptr<uint8_t, FreeDel> out((uint8_t *)alloc_rows_out(out_cap));  // freed on every error return
  if (!out) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
  RowCursor cur{0, 0, 0};
  u64 state = 0;
  double d2h = 0;
  for (u64 k = 0; k < K; ++k) {
    HIPCHK(hipStreamWaitEvent(s, ev[(lay.lo(k) + lay.end(k) - 1) / PIPE_SLAB], 0), "wait slab");
    DevResult dr;
    shockidx_result r2;
    reset_result(&r2);
    u64 row_base = 0;
    const int rc = index_slab(c, lay, k, c->d_in + lay.lo(k), F_FASTQ, 0, state, cur.total, rcap - cur.total, false, &dr, &r2, &row_base);
    if (rc < 0) return forward_error(res, r2, rc);
    res->kernel_ms += r2.kernel_ms;
    res->index_ms += r2.index_ms;
    if (classify(rc, dr, row_base, lay.last(k), false) != SlabOutcome::Clean) {
      out.reset();
      return plain();
    }
    const u64 owned = dr.count - row_base;
    if ((cur.total + owned) * 16 > out_cap) {
      size_t nc = out_cap;
      while ((cur.total + owned) * 16 > nc) nc *= 2;
      uint8_t *o2 = (uint8_t *)realloc(out.get(), nc);
      if (!o2) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
      (void)out.release();
      out.reset(o2);
      out_cap = nc;
    }
    const double td = now_ms();
    uint8_t *dst = out.get() + cur.total * 16;
    if (int rc2 = rows_to_host(c, c->d_rows + 2 * cur.total, owned * 16, dst, s, res)) return rc2;
    d2h += now_ms() - td;
    // the slab continues the table (record.go:51-83)
    if (!cur.accept((const u64 *)dst, owned, true)) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_SEAM_MSG);
    state = dr.state_out;
  }
  // the table ends at the file end, or before trailing blank lines (fastq.go:141-156)
  const uint8_t *hb = (const uint8_t *)data;
  if (!table_ends_at_file_end(F_FASTQ, cur.next_off, n, cur.last_len, [&](u64 off, uint8_t *b) { *b = hb[off]; return true; }))
    return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_END_MSG);
  if (cur.total * 16 < out_cap) {
    uint8_t *o2 = (uint8_t *)realloc(out.get(), cur.total ? cur.total * 16 : 16);
    if (o2) {
      (void)out.release();
      out.reset(o2);
    }
  }
  *rows = (uint64_t *)out.release();
  res->count = cur.total;
  res->format = SHOCKIDX_FMT_FASTQ;
  res->status = SHOCKIDX_OK;
  res->path = 3;  // the slab pipeline (the plain fallback reports its device build's path)
  res->d2h_ms = d2h;
  res->total_ms = now_ms() - t0;
  res->h2d_ms = res->total_ms - d2h - res->kernel_ms;  // the rest is waiting for the PCIe stream
  return SHOCKIDX_OK;
}

}  // namespace sidx_host
