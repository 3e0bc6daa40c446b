// sidx_walk.hpp -- what the file-level slab walks share: the record pipelines (sidx_pipeline.cpp)
// and the carried-state walks of the column, subset and chunkrecord indexes (sidx_walks.cpp, which
// also defines the functions declared here).  The arrival events, the page-cache source, the
// two-slot stage, the row drain, the file-range load and the timing epilogue, each written once.
// Internal: not part of the C ABI (include/shockidx.h).
#pragma once
#include <stdlib.h>
#include <sys/mman.h>

#include <functional>
#include <vector>

#include "sidx_host.hpp"

namespace sidx_host {

// the slab builds' end-of-build invariants (never expected: a violation is an internal error,
// not a short table)
const char *const SLAB_SEAM_MSG = "internal error: a slab's first row does not start where the previous slab's rows end";
const char *const SLAB_END_MSG = "internal error: the rows do not end at the end of the file";

// One arrival event per slab, recorded on the copy stream.  Destroyed only once the copy stream
// has drained: declare it before whatever issues copies, so that it is destroyed after it.
struct SlabEvents {
  std::vector<hipEvent_t> ev;
  hipStream_t copy_stream;
  SlabEvents(sidx::u64 K, hipStream_t cs) : ev(K, nullptr), copy_stream(cs) {}
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
  typedef sidx::u64 u64;

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

// The two slots of a carried-state walk over an n-byte file: slab k + 1 is copied into the other
// slot on the copy stream while slab k runs on the compute stream.  Owns the two arrival events
// and the source, the events first: they outlive the source's copies.
struct TwoSlots {
  shockidx_ctx *c;
  Err res;
  SlabEvents events;
  PageCacheSource src;
  // (the n bytes from file offset `off` on: a whole file, or the section a filtered download reads)
  TwoSlots(shockidx_ctx *ctx, int fd, sidx::u64 off, sidx::u64 n, Err r)
      : c(ctx), res(r), events(2, ctx->s_copy), src(ctx, fd, off, n, r) {}
  // section bytes [lo, hi) to offset d of slot i, their arrival recorded in the slot's event (an
  // empty range copies nothing and still records it)
  int stage(int i, sidx::u64 d, sidx::u64 lo, sidx::u64 hi) {
    if (int rc = src.copy_range(c->d_slot[i] + d, lo, hi, lo)) return rc;
    HIPCHK(hipEventRecord(events.ev[i], c->s_copy), "event");
    return 0;
  }
  // the compute stream waits for what was staged into slot i
  int wait(int i) {
    HIPCHK(hipStreamWaitEvent(c->stream, events.ev[i], 0), "wait slab");
    return 0;
  }
  // after the walk, before the pages are unpinned and unmapped: every copy has landed.  The walk's
  // code rc, or the drain's error when the walk has none of its own.
  int finish(int rc) {
    const hipError_t se = src.drain();
    if (se != hipSuccess && rc >= 0 && rc != SHOCKIDX_EFORMAT) rc = set_hip(res, se, "H2D sync");
    return rc;
  }
};

// What a walk needs of the context before its first copy: the copy stream and, with rows = true,
// the two pinned row buffers (h_rows[0] for rows on their way out, h_rows[1] for file bytes on
// their way in).
int walk_prereqs(shockidx_ctx *c, Err res, bool rows = true);

// m rows of the device table d_tab into the sink as rows first, first + 1, ...: through the pinned
// buffer c->h_rows[0] in chunks of 4 Mi rows, each waited for on c->stream before it is put, so
// one buffer serves (no copy overlaps a put).  each(rows, k, done), when given, sees every chunk on
// the host before its put (k rows, after `done` earlier ones): it may check or rewrite them, and a
// code other than 0 ends the drain.  *t_d2h (when given) grows by the time a whole drain took.
typedef std::function<int(sidx::u64 *rows, sidx::u64 k, sidx::u64 done)> RowChunkFn;
int drain_rows(shockidx_ctx *c, const sidx::u64 *d_tab, sidx::u64 m, sidx::u64 first, RowSink &sink,
               const RowChunkFn &each, double *t_d2h, Err res);

// File bytes [off, off + total) of fd to device memory at dst: pread into c->h_rows[1], 64 MiB at
// a time, each piece copied on c->stream and waited for.  The caller's texts: a read error is
// read_prefix + strerror, a file that ends early short_msg, a failed copy names copy_what.
int file_to_device(shockidx_ctx *c, int fd, sidx::u64 off, sidx::u64 total, uint8_t *dst, const char *read_prefix,
                   const char *short_msg, const char *copy_what, Err res);

// total bytes of device memory at d_src to the descriptor out_fd, in order: through the pinned
// buffer c->h_rows[0], 64 MiB at a time, each piece waited for on c->stream and then written with
// write(2) -- out_fd may be a pipe or a socket (no lseek, no pwrite); short writes and EINTR are
// handled, and a reader that has gone away is EPIPE here, not a signal.  A failed write is
// SHOCKIDX_EIO with the errno text.  *t_d2h / *t_write grow by the time the copies / writes took.
int drain_bytes(shockidx_ctx *c, const uint8_t *d_src, sidx::u64 total, int out_fd, double *t_d2h, double *t_write,
                Err res);

// count, format, path and the times of a walk that ends here (t0: when it began); what is neither
// row copy nor kernel is waiting for the PCIe stream
void finish_walk(shockidx_result *res, int kfmt, sidx::u64 total, sidx::u32 path, double kernel_ms, double index_ms,
                 double t_d2h, double t0);

}  // namespace sidx_host
