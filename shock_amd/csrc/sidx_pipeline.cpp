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
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_slabwalk.hpp"
#include "sidx_colwalk.hpp"
#include "sidx_chunkwalk.hpp"
#include "sidx_subwalk.hpp"
#include "sidx_launch.hpp"
#include "sidx_host.hpp"

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

// the slab builds' end-of-build invariants (never expected: a violation is an internal error,
// not a short table)
const char *const SLAB_SEAM_MSG = "internal error: a slab's first row does not start where the previous slab's rows end";
const char *const SLAB_END_MSG = "internal error: the rows do not end at the end of the file";

// One arrival event per slab, recorded on the copy stream.  Destroyed only once the copy stream
// has drained: declare it before whatever issues copies, so that it is destroyed after it.
struct SlabEvents {
  std::vector<hipEvent_t> ev;
  hipStream_t copy_stream;
  SlabEvents(u64 K, hipStream_t cs) : ev(K, nullptr), copy_stream(cs) {}
  hipError_t create() {
    for (auto &e : ev)
      if (hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming)) return rc;
    return hipSuccess;
  }
  ~SlabEvents() {
    (void)hipStreamSynchronize(copy_stream);
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

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

// Node bytes to device memory on the copy stream.  (a) DMA straight out of the page cache: the
// file mapped read-only and pinned 256 MiB at a time (hipHostRegister of page-cached pages runs at
// ~160 GB/s, ahead of PCIe), so the bytes cross the host's memory once instead of being copied
// into pinned staging first (tools/probes/regprobe.cpp: register 6.7 ms + H2D 18.7 ms per GiB).
// Chunks stay pinned until the copy stream drains (unpinning behind the DMA cost a quarter of the
// rate, profiles/r04/e2e_fd_page_cache_dma.txt) -- unless the process-wide pin budget runs out,
// when the ring unpins the chunks behind its current slab.  (b) When the file does not map or its
// pages do not pin: the copy threads pread it into the two pinned staging buffers.
// Lifetime: the copy stream must have drained before a chunk is unpinned or the file unmapped, so
// the destructor drains it first (drain() does, and reports the error); and the slabs' arrival
// events outlive this object (SlabEvents is declared before it).
class PageCacheSource {
 public:
  PageCacheSource(shockidx_ctx *c, int fd, u64 base, u64 n, Err res)
      : c_(c), res_(res), a0_(base & ~4095ull), lead_(base - a0_), mn_(lead_ + n),
        maplen_((size_t)((mn_ + 4095) & ~4095ull)), pinned_((mn_ + CH - 1) / CH, 0), fill_{fd, res, c->pool} {
    if (!getenv("SHOCKIDX_NO_MMAP_DMA")) {
      void *mp = mmap(nullptr, maplen_, PROT_READ, MAP_SHARED, fd, (off_t)a0_);
      if (mp != MAP_FAILED) map_ = (uint8_t *)mp;
    }
    pin_ok_ = map_ != nullptr;
  }
  ~PageCacheSource() {
    if (!drained_) (void)hipStreamSynchronize(c_->s_copy);
    for (u64 j = 0; j < pinned_.size(); ++j) unpin(j);
    if (map_) munmap(map_, maplen_);
  }
  PageCacheSource(const PageCacheSource &) = delete;
  // every copy issued so far has landed
  hipError_t drain() {
    drained_ = true;
    return hipStreamSynchronize(c_->s_copy);
  }
  // node bytes [a, b) to device address dst: pinned chunks, else staging.  keep_from: the chunks
  // wholly before this node byte may be unpinned when the pin budget runs out
  int copy_range(uint8_t *dst, u64 a, u64 b, u64 keep_from) {
    const Err res = res_;
    a += lead_;  // (map coordinates from here: file offset a0 + x)
    b += lead_;
    keep_from += lead_;
    while (a < b) {
      const u64 j = a / CH, ce = (j + 1) * CH < b ? (j + 1) * CH : b;
      if (pin(j, keep_from)) {
        if (hipError_t e = hipMemcpyAsync(dst, map_ + a, ce - a, hipMemcpyHostToDevice, c_->s_copy)) return set_hip(res, e, "page-cache DMA");
        dst += ce - a;
        a = ce;
        continue;
      }
      const size_t k = ce - a < STAGE_BYTES ? (size_t)(ce - a) : STAGE_BYTES;
      HIPCHK(hipEventSynchronize(c_->stage_ev[stage_i_]), "stage wait");  // buffer free again
      if (int rc = fill_(c_->h_stage[stage_i_], a0_ + a, k)) return rc;
      hipError_t e;
      if ((e = hipMemcpyAsync(dst, c_->h_stage[stage_i_], k, hipMemcpyHostToDevice, c_->s_copy)) != hipSuccess ||
          (e = hipEventRecord(c_->stage_ev[stage_i_], c_->s_copy)) != hipSuccess)
        return set_hip(res, e, "H2D");
      stage_i_ ^= 1;
      dst += k;
      a += k;
    }
    return 0;
  }

 private:
  static constexpr u64 CH = 256ull << 20;  // (chunks in map coordinates)
  size_t chunk_len(u64 j) const { return (size_t)((((j * CH + CH < mn_ ? j * CH + CH : mn_) + 4095) & ~4095ull) - j * CH); }
  void unpin(u64 j) {
    if (!pinned_[j]) return;
    (void)hipHostUnregister(map_ + j * CH);
    pin_release(pinned_[j]);
    pinned_[j] = 0;
  }
  // pin chunk j (reserving its bytes); false: it does not pin (the caller stages instead)
  bool pin(u64 j, u64 keep_from) {
    if (pinned_[j]) return true;
    if (!pin_ok_) return false;
    const u64 len = chunk_len(j);
    if (!pin_reserve(len)) {
      // over the process-wide budget: unpin the chunks wholly before keep_from (their copies
      // must have landed first), then try once more
      bool any = false;
      for (u64 i = 0; i < j && (i + 1) * CH <= keep_from; ++i) any |= pinned_[i] != 0;
      if (!any || hipStreamSynchronize(c_->s_copy) != hipSuccess) return false;
      for (u64 i = 0; i < j && (i + 1) * CH <= keep_from; ++i) unpin(i);
      if (!pin_reserve(len)) return false;
    }
    if (hipHostRegister(map_ + j * CH, len, 0) != hipSuccess) {
      (void)hipGetLastError();
      pin_release(len);
      pin_ok_ = false;
      return false;
    }
    pinned_[j] = len;
    return true;
  }
  shockidx_ctx *c_;
  Err res_;
  const u64 a0_, lead_, mn_;  // the file from the page below base: node byte a is map[lead + a]
  const size_t maplen_;
  uint8_t *map_ = nullptr;
  std::vector<u64> pinned_;  // bytes registered (and reserved) per chunk
  bool pin_ok_ = false;      // chunks still pin (else the staging path from here on)
  bool drained_ = false;
  int stage_i_ = 0;
  PreadFill fill_;
};

// A slab's owned rows (device rows [0, owned)) D2H through the two pinned row buffers into the
// sink: chunk j + 1's DMA overlaps chunk j's sink.  0, or the library code (message in o.cres).
int rows_to_sink(Walk &w, WalkResult &o, u64 owned) {
  shockidx_ctx *c = w.c;
  const double td = now_ms();
  const u64 per = STAGE_BYTES / 16;
  u64 done_rows = 0;
  int b = 0;
  while (done_rows < owned) {
    const u64 m = owned - done_rows < per ? owned - done_rows : per;
    if (hipMemcpyAsync(c->h_rows[b], c->d_rows + 2 * done_rows, m * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return set_msg(&o.cres, SHOCKIDX_EHIP, "rows copy");
    // the slab's rows continue the table (record.go:51-83): its first row starts where the
    // previous slab's last row ended
    const u64 at = o.cur.total;
    if (!o.cur.accept((const u64 *)c->h_rows[b], m, done_rows == 0)) return set_msg(&o.cres, SHOCKIDX_EINTERNAL, SLAB_SEAM_MSG);
    if (int r = w.sink.put(c->h_rows[b], at, m, &o.cres)) return r;
    done_rows += m;
    b ^= 1;
  }
  o.t_d2h += now_ms() - td;
  return 0;
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
    if (int e = rows_to_sink(w, o, dr.count - row_base)) return o.fail(e);
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

// count, format, path and the times of a walk that ends here
void finish_walk(shockidx_result *res, int kfmt, u64 total, u32 path, const shockidx_result &cres, double t_d2h,
                 double t0) {
  res->count = total;
  res->format = kfmt == F_LINE ? SHOCKIDX_FMT_LINE : kfmt;
  res->path = path;
  res->kernel_ms = cres.kernel_ms;
  res->index_ms = cres.index_ms;
  res->d2h_ms = t_d2h;
  res->total_ms = now_ms() - t0;
  res->h2d_ms = res->total_ms - t_d2h - res->kernel_ms;  // the rest is waiting for the PCIe stream
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
  const double td = now_ms();
  const u64 per = STAGE_BYTES / 16;
  for (u64 d = 0; d < r3.count;) {
    const u64 m = r3.count - d < per ? r3.count - d : per;
    HIPCHK(hipMemcpyAsync(c->h_rows[0], c->d_rows + 2 * d, m * 16, hipMemcpyDeviceToHost, s), "rows copy");
    HIPCHK(hipStreamSynchronize(s), "rows copy");
    u64 *hr = (u64 *)c->h_rows[0];
    for (u64 i = 0; i < m; ++i) hr[2 * i] += r;
    const u64 at = o.cur.total;
    if (!o.cur.accept(hr, m, d == 0)) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_SEAM_MSG);
    if (int e = w.sink.put(c->h_rows[0], at, m, res)) return e;
    d += m;
  }
  o.cres.kernel_ms += r3.kernel_ms;
  o.cres.index_ms += r3.index_ms;
  finish_walk(res, r3.format, o.cur.total, 4, o.cres, o.t_d2h + (now_ms() - td), t0);
  forward_error(res, r3, r3.status);
  res->reruns = r3.reruns + 1;
  return rc;
}

// A Go error in a slab: the rows before it are in the sink; its text as the one-pass build
// reports it.  The FASTA piece is read back from the file (it may begin before the slot holding
// the slab).
int finish_go_error(Walk &w, WalkResult &o, shockidx_result *res, double t0) {
  finish_walk(res, o.kfmt, o.cur.total, 4, o.cres, o.t_d2h, t0);
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
  if (!c->s_copy) HIPCHK(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking), "copy stream");
  for (int i = 0; i < 2; ++i)
    if (!c->h_rows[i]) HIPCHK(hipHostMalloc(&c->h_rows[i], STAGE_BYTES, 0), "hipHostMalloc(rows)");
  const u64 SLOT = RING_FRONT + lay.S + PIPE_HALO + 64;  // (kept by the context, like its other caches, until a trim)
  if (lay.ring) {
    if (c->d_slot[0].cap != SLOT || c->d_slot[1].cap != SLOT) {
      // the caches of earlier (larger) builds go first: the node buffer of a one-pass build, rows
      trim_workspace(c, 0);
      for (auto &slot : c->d_slot)
        if (int rc = slot.exact(SLOT, res)) return rc;
    } else if (c->d_in) {
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
        finish_walk(res, o.kfmt, o.cur.total, 4, o.cres, o.t_d2h, t0);
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
  finish_walk(res, o.kfmt, o.cur.total, ring ? 4 : 3, o.cres, o.t_d2h, t0);  // the slab pipeline (4: through the two slots)
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

// ---- the column index's walk -------------------------------------------------------------------
// CreateColumnIndex (column.go:53-108) slab by slab through two slots: slab k + 1 is copied on the
// copy stream (PageCacheSource: page-cache DMA, else the pinned staging, whose preads run on this
// thread) while slab k's kernels run, each slab's rows go to the sink as they are made, and the
// loop's state travels in the device carry.  sidx_colwalk.hpp holds the sizing and the one retry
// rule.  The device holds the two slots, the carry with one slab's workspace (c->d_colb) and one
// slab's rows, all exact-size.
namespace {

struct ColWalk {
  shockidx_ctx *c;
  u64 n, S, halo;
  SlabEvents &events;
  PageCacheSource &src;
  Err res;
  // slab p into slot i (its first byte at COLWALK_FRONT), its arrival recorded in events.ev[i]
  int stage(int i, const ColSlabPos &p) {
    if (int rc = src.copy_range(c->d_slot[i] + COLWALK_FRONT - p.front, p.lo - p.front, p.lo + p.end, p.lo - p.front)) return rc;
    if (hipError_t e = hipEventRecord(events.ev[i], c->s_copy)) return set_hip(res, e, "event");
    return 0;
  }
};

// the slab's m rows (device rows [0, m)) through the pinned row buffers into the sink; *next: the
// offset the table has reached (every row starts there: column.go:90-93)
int col_rows_to_sink(shockidx_ctx *c, u64 m, ColRowCursor &cur, u64 *next, RowSink &sink, double *t_d2h,
                     shockidx_result *res) {
  const double td = now_ms();
  const u64 per = STAGE_BYTES / 16;
  int b = 0;
  for (u64 done = 0; done < m; b ^= 1) {
    const u64 k = m - done < per ? m - done : per;
    HIPCHK(hipMemcpyAsync(c->h_rows[b], c->d_rows + 2 * done, k * 16, hipMemcpyDeviceToHost, c->stream), "rows copy");
    HIPCHK(hipStreamSynchronize(c->stream), "rows copy");
    const u64 *r = (const u64 *)c->h_rows[b];
    for (u64 i = 0; i < k; ++i) {
      if (r[2 * i] != *next) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_SEAM_MSG);
      *next += r[2 * i + 1];
    }
    if (int rc = sink.put(c->h_rows[b], cur.take(k), k, res)) return rc;
    done += k;
  }
  *t_d2h += now_ms() - td;
  return 0;
}

}  // namespace

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
  if (!c->s_copy) HIPCHK(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking), "copy stream");
  for (int i = 0; i < 2; ++i)
    if (!c->h_rows[i]) HIPCHK(hipHostMalloc(&c->h_rows[i], STAGE_BYTES, 0), "hipHostMalloc(rows)");
  const u64 slot = colwalk_slot_bytes(S, halo), ws_b = sidx_col_tile_bytes((S + TILE - 1) / TILE);
  u64 row_cap = colwalk_rows_cap(S);
  if (c->d_slot[0].cap != slot || c->d_slot[1].cap != slot || c->d_colb.cap != carry_b + ws_b || c->d_rows.cap != row_cap) {
    trim_workspace(c, 0);  // the caches of other builds go first
    for (auto &sl : c->d_slot)
      if (int rc = sl.exact(slot, res)) return rc;
    if (int rc = c->d_colb.exact(carry_b + ws_b, res)) return rc;
    if (int rc = c->d_rows.exact(row_cap, res)) return rc;
  }
  ColCarry *carry = c->d_colb.as<ColCarry>();
  void *ws = c->d_colb + carry_b;
  SlabEvents events(2, c->s_copy);  // (outlives the source's copies)
  HIPCHK(events.create(), "event");
  PageCacheSource src(c, fd, 0, n, res);
  ColWalk w{c, n, S, halo, events, src, res};
  ColRowCursor cur;
  u64 next = 0;
  double t_d2h = 0;
  int i = 0;
  ColSlabPos p = colwalk_slab_at(0, S, halo, n);
  int rc = w.stage(0, p);
  while (!rc) {
    bool more = !p.last;
    ColSlabPos q = p;
    if (more) {  // the slab expected next, on its way while this one is indexed
      q = colwalk_slab_at(p.lo + p.n, S, halo, n);
      if ((rc = w.stage(i ^ 1, q))) break;
    }
    if (hipError_t e = hipStreamWaitEvent(s, events.ev[i], 0)) { rc = set_hip(res, e, "wait slab"); break; }
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
    if (moved && (rc = w.stage(i ^ 1, q))) break;  // a fresh slot from where the shortened slab ends
    p = q;
    i ^= 1;
  }
  const hipError_t se = src.drain();  // before the pages are unpinned and unmapped
  if (se != hipSuccess && rc >= 0 && rc != SHOCKIDX_EFORMAT) rc = set_hip(res, se, "H2D sync");
  if (rc) {
    res->count = 0;  // (column.go:76 returns count 0; an error leaves no table)
    return rc;
  }
  if (cur.total && next != n) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_END_MSG);
  res->count = cur.total;
  res->index_ms = res->kernel_ms;
  res->d2h_ms = t_d2h;
  res->total_ms = now_ms() - t0;
  res->h2d_ms = res->total_ms - t_d2h - res->kernel_ms;
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

// m rows of a device table through a pinned buffer into a sink, numbered from `first`
int sub_table_to_sink(shockidx_ctx *c, const u64 *d_tab, u64 m, u64 first, RowSink &sink, Err res) {
  const u64 per = STAGE_BYTES / 16;
  for (u64 done = 0; done < m;) {
    const u64 k = m - done < per ? m - done : per;
    HIPCHK(hipMemcpyAsync(c->h_rows[0], d_tab + 2 * done, k * 16, hipMemcpyDeviceToHost, c->stream), "rows copy");
    HIPCHK(hipStreamSynchronize(c->stream), "rows copy");
    if (int rc = sink.put(c->h_rows[0], first + done, k, res)) return rc;
    done += k;
  }
  return 0;
}

// rows [w.row0, w.row0 + w.rows) of the parent index file into the window buffer
int sub_load_window(shockidx_ctx *c, int fd, const SubWindow &w, Err res) {
  const u64 per = STAGE_BYTES;
  for (u64 done = 0, total = 16 * w.rows; done < total;) {
    const u64 k = total - done < per ? total - done : per;
    for (u64 got = 0; got < k;) {
      const ssize_t r = pread(fd, c->h_rows[1] + got, k - got, (off_t)(16 * w.row0 + done + got));
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) return set_msg(res, SHOCKIDX_EIO, std::string("read: ") + strerror(errno));
      if (r == 0) return set_msg(res, SHOCKIDX_EIO, "read: the parent index file is shorter than its size");
      got += (u64)r;
    }
    HIPCHK(hipMemcpyAsync(c->d_spar + done, c->h_rows[1], k, hipMemcpyHostToDevice, c->stream), "window copy");
    HIPCHK(hipStreamSynchronize(c->stream), "window copy");
    done += k;
  }
  return 0;
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
  if (!c->s_copy) HIPCHK(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking), "copy stream");
  for (int i = 0; i < 2; ++i)
    if (!c->h_rows[i]) HIPCHK(hipHostMalloc(&c->h_rows[i], STAGE_BYTES, 0), "hipHostMalloc(rows)");
  const u64 slot = subwalk_slot_bytes(S, halo), rows_cap = subwalk_rows_cap(S), runs_cap = subwalk_runs_cap(S);
  u64 ends_b = 0, line_b = 0;  // a call's workspace, sized for the longest window so that no call grows it
  subset_slab_ws_parts(S + halo, &ends_b, &line_b);
  if (c->d_slot[0].cap != slot || c->d_slot[1].cap != slot || c->d_spar.cap != 16 * W || c->d_rows.cap != rows_cap ||
      c->d_sruns.cap != carry_b + 16 * runs_cap || c->d_sends.cap != ends_b || c->d_sub.cap != line_b) {
    trim_workspace(c, 0);  // the caches of other builds go first
    for (auto &sl : c->d_slot)
      if (int rc = sl.exact(slot, res)) return rc;
    if (int rc = c->d_spar.exact(16 * W, res)) return rc;
    if (int rc = c->d_rows.exact(rows_cap, res)) return rc;
    if (int rc = c->d_sruns.exact(carry_b + 16 * runs_cap, res)) return rc;
    if (int rc = c->d_sends.exact(ends_b, res)) return rc;
    if (int rc = c->d_sub.exact(line_b, res)) return rc;
  }
  SubCarry *carry = c->d_sruns.as<SubCarry>();
  u64 *d_runs = (u64 *)(c->d_sruns + carry_b);
  HIPCHK(hipMemsetAsync(carry, 0, carry_b, s), "carry");
  SlabEvents events(2, c->s_copy);  // (outlives the source's copies)
  HIPCHK(events.create(), "event");
  PageCacheSource src(c, ids_fd, 0, n, res);
  ColWalk w{c, n, S, halo, events, src, res};
  SubCursor cur;
  SubWindow win = subwalk_window_at(0, W, parent_count);
  int rc = sub_load_window(c, parent_fd, win, res);
  st.windows = 1;
  st.parent_bytes = 16 * win.rows;
  int i = 0;
  ColSlabPos p = colwalk_slab_at(0, S, halo, n);
  if (!rc) rc = w.stage(0, p);
  st.ids_bytes = p.end;
  shockidx_subset_slab_result r2;
  memset(&r2, 0, sizeof r2);
  while (!rc) {
    bool more = !p.last, moved = false;
    ColSlabPos q = p;
    if (more) {  // the slab expected next, on its way while this one runs
      q = colwalk_slab_at(p.lo + p.n, S, halo, n);
      if ((rc = w.stage(i ^ 1, q))) break;
      st.ids_bytes += q.end + q.front;
    }
    if (hipError_t e = hipStreamWaitEvent(s, events.ev[i], 0)) { rc = set_hip(res, e, "wait slab"); break; }
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
      if ((rc = sub_table_to_sink(c, c->d_rows, r2.rows, cur.take_rows(r2.rows), *sinks.rows, res))) break;
      if (want_runs && (rc = sub_table_to_sink(c, d_runs, r2.runs, cur.take_runs(r2.runs), *sinks.runs, res))) break;
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
      if ((rc = w.stage(i ^ 1, q))) break;
      st.ids_bytes += q.end + q.front;
    }
    p = q;
    i ^= 1;
  }
  const hipError_t se = src.drain();  // before the pages are unpinned and unmapped
  if (se != hipSuccess && rc >= 0 && rc != SHOCKIDX_EFORMAT) rc = set_hip(res, se, "H2D sync");
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
  if (!c->s_copy) HIPCHK(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking), "copy stream");
  for (int i = 0; i < 2; ++i)
    if (!c->h_rows[i]) HIPCHK(hipHostMalloc(&c->h_rows[i], STAGE_BYTES, 0), "hipHostMalloc(rows)");
  const u64 slot = chunkwalk_slot_bytes(S), cra = chunkwalk_cra_bytes(vmax, dv.scan_bytes, dv.gslot),
            crb = chunkwalk_crb_bytes(vmax, chunk), row_cap = chunkwalk_row_bound(vmax, chunk);
  if (c->d_slot[0].cap != slot || c->d_slot[1].cap != slot || c->d_cra.cap != cra || c->d_crb.cap != crb ||
      c->d_crc.cap != dv.carry_bytes || c->d_rows.cap != row_cap) {
    trim_workspace(c, 0);  // the caches of other builds go first
    for (auto &sl : c->d_slot)
      if (int rc = sl.exact(slot, res)) return rc;
    if (int rc = c->d_cra.exact(cra, res)) return rc;
    if (int rc = c->d_crb.exact(crb, res)) return rc;
    if (int rc = c->d_crc.exact(dv.carry_bytes, res)) return rc;
    if (int rc = c->d_rows.exact(row_cap, res)) return rc;
  }
  ChunkCarry *carry = c->d_crc.as<ChunkCarry>();
  SlabEvents events(2, c->s_copy);  // (outlives the source's copies)
  HIPCHK(events.create(), "event");
  PageCacheSource src(c, fd, 0, n, res);
  auto stage = [&](u64 k) -> int {  // slab k into slot k mod 2, its arrival recorded in that slot's event
    const ChunkSlot p = chunkwalk_slot(k, S, n);
    if (p.hi > p.lo)
      if (int rc = src.copy_range(c->d_slot[k & 1], p.lo, p.hi, p.lo)) return rc;
    if (hipError_t e = hipEventRecord(events.ev[k & 1], c->s_copy)) return set_hip(res, e, "event");
    return 0;
  };
  const u64 K = chunkwalk_slots(S, n);
  ColRowCursor cur;
  u64 next = 0;
  double t_d2h = 0;
  int kfmt = 0;
  int rc = stage(0);
  for (u64 k = 0; !rc && k < K; ++k) {
    if (k + 1 < K && (rc = stage(k + 1))) break;  // the next slab, on its way while this one is walked
    if (hipError_t e = hipStreamWaitEvent(s, events.ev[k & 1], 0)) { rc = set_hip(res, e, "wait slab"); break; }
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
  const hipError_t se = src.drain();  // before the pages are unpinned and unmapped
  if (se != hipSuccess && rc >= 0 && rc != SHOCKIDX_EFORMAT) rc = set_hip(res, se, "H2D sync");
  if (rc) {
    res->count = 0;
    return rc;
  }
  if (next != n) return set_msg(res, SHOCKIDX_EINTERNAL, SLAB_END_MSG);
  res->count = cur.total;
  res->index_ms = res->kernel_ms;
  res->d2h_ms = t_d2h;
  res->total_ms = now_ms() - t0;
  res->h2d_ms = res->total_ms - t_d2h - res->kernel_ms;
  res->status = SHOCKIDX_OK;
  return SHOCKIDX_OK;
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
  if (!c->s_copy) HIPCHK(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking), "copy stream");
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
