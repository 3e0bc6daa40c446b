// sidx_build.cpp -- one device-resident index build and what it needs on the host: the context's
// grow-only device workspaces, format resolution and speculation, the index pass itself
// (run_index), the device result turned into Go's (count, err), staging of host memory and file
// bytes into HBM, and the table copy-out through the pinned staging buffers.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_subset.hpp"
#include "sidx_launch.hpp"
#include "sidx_host.hpp"

using namespace sidx;

namespace sidx_host {

CopyPool::CopyPool(int n) : nt_(n) {
  for (int i = 0; i < n; ++i) th_.emplace_back([this, i] { run(i); });
}
CopyPool::~CopyPool() {
  {
    std::lock_guard<std::mutex> g(m_);
    stop_ = true;
    ++gen_;
  }
  cv_.notify_all();
  for (auto &t : th_) t.join();
}
void CopyPool::copy(void *dst, const void *src, size_t n) {
  uint8_t *d = (uint8_t *)dst;
  const uint8_t *sp = (const uint8_t *)src;
  parallel(n, [d, sp](size_t a, size_t b) { memcpy(d + a, sp + a, b - a); });
}
void CopyPool::parallel(size_t n, const std::function<void(size_t, size_t)> &f) {
  if (n < (4u << 20) || nt_ < 2) {
    if (n) f(0, n);
    return;
  }
  std::unique_lock<std::mutex> lk(m_);
  fn_ = &f;
  n_ = n;
  pending_ = nt_;
  ++gen_;
  cv_.notify_all();
  done_.wait(lk, [this] { return pending_ == 0; });
}
void CopyPool::run(int i) {
  unsigned long long seen = 0;
  for (;;) {
    const std::function<void(size_t, size_t)> *f;
    size_t n;
    {
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&] { return gen_ != seen; });
      seen = gen_;
      if (stop_) return;
      f = fn_;
      n = n_;
    }
    const size_t per = ((n + nt_ - 1) / nt_ + 4095) & ~(size_t)4095;
    const size_t a = (size_t)i * per < n ? (size_t)i * per : n, b = a + per < n ? a + per : n;
    if (b > a) (*f)(a, b);
    std::lock_guard<std::mutex> g(m_);
    if (--pending_ == 0) done_.notify_one();
  }
}

constexpr u64 SPEC_MIN_BYTES = 1ull << 20;  // smaller AUTO builds detect first (a re-run costs little)

int set_hip(Err r, hipError_t e, const char *what) {
  return set_msg(r, SHOCKIDX_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

bool verify_rows() {
  const char *v = getenv("SHOCKIDX_VERIFY");
  return v && *v && strcmp(v, "0") != 0;
}

// dev knob (placement probes): SHOCKIDX_CONTIG_WS bit 1 = the tile status words, bit 2 = the tile
// pass's record-start slots in contiguous memory
static bool ws_contig(int bit) {
  const char *e = getenv("SHOCKIDX_CONTIG_WS");
  return e && (atoi(e) & bit);
}

// free the large caches (they regrow on demand); the tile block goes only with keep = 0, or when
// the rest is still over keep
void trim_workspace(shockidx_ctx *c, u64 keep) {
  if (c->bufs.trim(keep, [c] { (void)hipStreamSynchronize(c->stream); })) c->last_spans = false;
}
int exact_workspace(shockidx_ctx *c, std::initializer_list<BufSet::Want> want, Err res) {
  auto quiesce = [c] {  // (called when the trim acts, as in trim_workspace)
    (void)hipStreamSynchronize(c->stream);
    c->last_spans = false;
  };
  return c->bufs.exact(want, quiesce, res);
}

// test hook: every status word published (INC) with the next build's epoch and payload 0, on
// the build stream -- the stale look-back words a recycled allocation could hold
static hipError_t poison_status(shockidx_ctx *c) {
  const u64 w = FLAG_INC | ((u64)((c->epoch + 1) & EPOCH_MASK) << EPOCH_SHIFT);
  std::vector<u64> h(c->d_status.cap, w);
  hipError_t e = hipMemcpyAsync(c->d_status, h.data(), h.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream);
  return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

// The tile block for ntiles tiles: the three buffers grow together (c->tiles_cap() tiles), and a
// build never sees a part of it -- whatever fails, the whole block is dropped.
static int ensure_tiles(shockidx_ctx *c, u64 ntiles, Err res) {
  if (c->tiles_cap() >= ntiles && c->d_status) return 0;
  // the fresh array is zeroed, so any epoch >= 1 is unpublished; the epoch keeps counting so
  // the first-bad / counter slots keep alternating (finalize resets the next build's slot)
  c->bufs.drop(BufClass::Tile);
  const u64 want = ntiles + ntiles / 8 + 64;
  auto fresh = [&]() -> int {
    // the status block: STATUS_ARRAYS words per tile (StatusArray, sidx_host.hpp)
    c->d_status.node = ws_contig(1);
    if (int rc = c->d_status.exact(STATUS_ARRAYS * want, res)) return rc;
    // detail slots: one per tile (+1) and one per k_fixup queue item (the FASTA tile pass)
    if (int rc = c->d_detail.exact(4 * want, res)) return rc;
    if (int rc = c->d_fix.exact(4 * want, res)) return rc;
    // on the build stream and waited for: a null-stream memset is not ordered with the
    // non-blocking context stream, and a reused allocation's old look-back words could be read
    if (c->inject & 1) HIPCHK(poison_status(c), "poison");
    HIPCHK(hipMemsetAsync(c->d_status, 0, c->d_status.bytes(), c->stream), "hipMemset(status)");
    if (c->inject & 2) HIPCHK(poison_status(c), "poison");
    HIPCHK(hipStreamSynchronize(c->stream), "hipMemset(status) sync");
    return 0;
  };
  const int rc = fresh();
  if (rc) c->bufs.drop(BufClass::Tile);
  return rc;
}

// resolve kind/fmt into the kernel format (device detection when AUTO).  With `gate`, an AUTO
// record build of a context whose last detection found FASTQ or FASTA speculates that format:
// k_detect is launched without waiting for it, *gate points at its result and the pipeline's
// kernels run only if it matches (SlabParams::gate); one host round trip per build instead of two.
int resolve_format(shockidx_ctx *c, const uint8_t *d_data, u64 n, int kind, int fmt, hipStream_t s,
                   int *kfmt, Err res, const int **gate) {
  if (gate) *gate = nullptr;
  if (kind == SHOCKIDX_LINE) { *kfmt = F_LINE; return 0; }
  if (kind != SHOCKIDX_RECORD) return set_msg(res, SHOCKIDX_EINVAL, "invalid index kind");
  if (fmt == SHOCKIDX_FMT_AUTO) {
    int *d_det = (int *)(c->d_small + SMALL_DETECT);
    HIPCHK(sidx_launch_detect(d_data, n, d_det, s), "detect launch");
    if (gate && n >= SPEC_MIN_BYTES && (c->spec_fmt == SHOCKIDX_FMT_FASTQ || c->spec_fmt == SHOCKIDX_FMT_FASTA)) {
      *gate = d_det;
      *kfmt = c->spec_fmt;
      return 0;
    }
    HIPCHK(hipMemcpyAsync(c->h_det, d_det, 2 * sizeof(int), hipMemcpyDeviceToHost, s), "detect copy");
    HIPCHK(hipStreamSynchronize(s), "detect sync");
    fmt = c->h_det[0];
    c->spec_fmt = fmt;
    if (fmt == SHOCKIDX_FMT_NONE) {
      // errors.go:20 via multi.go:61
      return set_msg(res, SHOCKIDX_EFORMAT, "Invalid file type for filter");
    }
  }
  if (fmt != SHOCKIDX_FMT_FASTA && fmt != SHOCKIDX_FMT_FASTQ && fmt != SHOCKIDX_FMT_SAM && fmt != SHOCKIDX_FMT_LINE)
    return set_msg(res, SHOCKIDX_EINVAL, "invalid format");
  *kfmt = fmt;
  return 0;
}

// After a gated build: the speculation was wrong (RF_MISSPEC) -> the detected format, or Go's
// error for none.  Returns 2 when the caller must re-run with *kfmt (0: the speculation held).
int respeculate(shockidx_ctx *c, const DevResult &dr, int *kfmt, shockidx_result *res) {
  if (!(dr.flags & RF_MISSPEC)) return 0;
  const int det = (int)dr.detected;
  c->spec_fmt = det;
  res->format = SHOCKIDX_FMT_NONE;
  if (det == SHOCKIDX_FMT_NONE) return set_msg(res, SHOCKIDX_EFORMAT, "Invalid file type for filter");
  if (det != SHOCKIDX_FMT_FASTA && det != SHOCKIDX_FMT_FASTQ && det != SHOCKIDX_FMT_SAM)
    return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: detected format");
  *kfmt = det;
  res->format = det;
  return 2;
}

const char *status_message(uint32_t code) {
  switch (code) {
    case ST_FQ_TRUNC: return "Invalid format: truncated fastq record";
    case ST_FQ_EMPTYLINES: return "Invalid format: empty line(s) between records";
    case ST_FQ_NOAT: return "Invalid format: id line does not start with @";
    case ST_FQ_NOID: return "Invalid format: missing sequence ID";
    case ST_FQ_EMPTYSEQ: return "Invalid format: empty sequence";
    case ST_FQ_NOPLUS: return "Invalid format: plus line does not start with +";
    case ST_FQ_IDMISMATCH: return "Invalid format: quality ID does not match sequence ID";
    case ST_FQ_LENMISMATCH: return "Invalid format: length of sequence and quality lines do not match";
    default: return nullptr;
  }
}

std::mutex &device_mutex(int device) {
  static std::mutex mu[64];
  return mu[device & 63];
}

// SHOCKIDX_{FA,LINE,SAM}_MODE=two (or 0): two-pass instead of the tile pass; read per build, for in-process A/B
static bool forced_two_pass(const char *envname) {
  const char *e = getenv(envname);
  return e && (!strcmp(e, "two") || !strcmp(e, "0"));
}

// The build path of one slab.  Tile passes (one read of the input): FASTQ, FASTA (detail slots of
// tiles + queue items within the key) and line, single builds and slabs alike; SAM single builds
// (slabs keep their halo handling).  Otherwise the two-pass build (k_tile_agg + scan + k_index1).
static TilePass choose_pass(const shockidx_ctx *c, int kfmt, u64 n, const SlabGeom *geom, bool general) {
  if (general || !c->d_fix) return TP_TWO_PASS;  // (no k_fixup queue: k_index1 for every format)
  if (kfmt == F_FASTQ) return TP_FQ;
  const bool fa_key_fits = 2 * c->tiles_cap() < (1ull << KEY_TILE_BITS);
  if (kfmt == F_FASTA && (!geom || n > 0) && !forced_two_pass("SHOCKIDX_FA_MODE") && fa_key_fits) return TP_FA;
  if (kfmt == F_LINE && n > 0 && !forced_two_pass("SHOCKIDX_LINE_MODE")) return TP_LINE;
  if (kfmt == F_SAM && n > 0 && !geom && !forced_two_pass("SHOCKIDX_SAM_MODE")) return TP_SAM;
  return TP_TWO_PASS;
}

// One device-resident index pass.  Fills *dr (host copy of the device result).
int run_index(shockidx_ctx *c, const uint8_t *d_data, u64 n, int kfmt, u64 *d_rows, u64 row_cap,
              hipStream_t s, DevResult *dr, shockidx_result *res, const SlabGeom *geom, bool general,
              const int *gate) {
  const u64 ntiles = n ? (n + TILE - 1) / TILE : 1;
  if (ntiles >= (1ull << KEY_TILE_BITS)) return set_msg(res, SHOCKIDX_EINVAL, "input too large for one slab");
  if (int rc = ensure_tiles(c, ntiles, res)) return rc;
  const TilePass pass = choose_pass(c, kfmt, n, geom, general);
  if (pass != TP_TWO_PASS) {  // the tile pass's staged positions and per-tile results
    const u64 words = sidx_tile_stage_words(pass, ntiles, c->tiles_grid);
    c->d_tile_stage.node = ws_contig(2);
    if (int rc = c->d_tile_stage.ensure(words, res)) return rc;
    if (int rc = c->d_tile_words.ensure(ntiles * FQ_TILE_WORDS, res)) return rc;
    if (pass == TP_FQ && c->want_spans)
      if (int rc = c->d_fqlines.ensure(ntiles * 3 * (TILE / 64), res)) return rc;
  }
  if (getenv("SHOCKIDX_TIMING") && !c->d_timing) {
    HIPCHK(hipMalloc(&c->d_timing, 9 * 8 * 65536), "hipMalloc(timing)");
  }
  // A build that stopped between taking its epoch and its finalize (a launch or sync error)
  // left its first-bad / counter slot, scan tickets included, unreset: reset both slots before
  // anything reads them (k_scan_excl would otherwise wait on look-back words nobody writes).
  if (c->slots_dirty) {
    HIPCHK(hipMemsetAsync(c->d_small + SMALL_BADKEY, 0xFF, 16, s), "slot reset");
    HIPCHK(hipMemsetAsync(c->d_small + SMALL_COUNTERS, 0, 2 * 4 * NCOUNTERS, s), "slot reset");
    c->slots_dirty = false;
  }
  // next epoch (taken only once every allocation above succeeded); when the 14-bit epoch wraps,
  // clear the status array so no stale word can carry the current epoch
  if (++c->epoch > EPOCH_MASK) {
    HIPCHK(hipMemsetAsync(c->d_status, 0, c->d_status.bytes(), s), "status clear");
    c->epoch = 2;  // keep the slot parity alternating across the wrap (EPOCH_MASK is odd)
  }
  c->slots_dirty = true;  // until this build's finalize has run (the sync below)
  const u32 slot = c->epoch & 1;
  SlabParams p;
  memset(&p, 0, sizeof p);
  p.data = d_data;
  p.n = n;
  p.end = geom ? geom->end : n;
  p.front = geom ? geom->front : 0;
  p.base = geom ? geom->base : 0;
  p.state_in = geom ? geom->state_in : 0;
  p.row_base = geom ? geom->row_base : 0;
  p.summary = geom ? (u64 *)geom->d_summary : nullptr;
  p.row_cap = row_cap;
  p.rows = d_rows;
  auto status_array = [c](StatusArray a) { return c->d_status + (u64)a * c->tiles_cap(); };
  p.status = status_array(SA_STATUS);
  p.pcnt = status_array(SA_PCNT);
  p.ppre = status_array(SA_PPRE);
  for (int i = 0; i < 2; ++i) p.scan_look[i] = status_array((StatusArray)(SA_LOOK0 + i));
  p.tile_agg = status_array(SA_TILE_AGG);
  p.tile_excl = status_array(SA_TILE_EXCL);
  p.pgrid = c->tiles_grid < ntiles ? c->tiles_grid : (u32)ntiles;
  p.fix = general ? nullptr : c->d_fix.get();  // null: the two-pass build (k_index1) for every format
  p.fixcap = (u32)c->tiles_cap();
  p.grid_cap = c->grid_cap;
  p.badkey = (u64 *)(c->d_small + SMALL_BADKEY + 8 * slot);
  p.badkey_next = (u64 *)(c->d_small + SMALL_BADKEY + 8 * (slot ^ 1));
  p.detail = c->d_detail;
  p.counters = (u32 *)(c->d_small + SMALL_COUNTERS + 4 * NCOUNTERS * slot);
  p.counters_next = (u32 *)(c->d_small + SMALL_COUNTERS + 4 * NCOUNTERS * (slot ^ 1));
  p.ntiles = (u32)ntiles;
  p.epoch = c->epoch;
  p.seq = geom ? geom->seq : 0;
  p.inject = (c->inject & 4) ? 1u : 0u;
  p.eof = geom ? geom->eof : 1;
  p.file_start = geom ? geom->file_start : 1;
  p.gate = gate;
  p.gate_fmt = kfmt;  // (also the format the two-pass launch instantiates)
  if (const char *dbg = getenv("SHOCKIDX_DEBUG")) p.debug = (u32)atoi(dbg);  // SIDX_DIAG variant ablations
  if (getenv("SHOCKIDX_TIMING")) {  // diagnostic phase timing: per-workgroup cycle sums
    HIPCHK(hipMemsetAsync(c->d_timing, 0, 9 * 8 * 65536, s), "timing clear");
    p.timing = c->d_timing;
  }
  DevResult *d_res = (DevResult *)(c->d_small + SMALL_RESULT);
  const bool tile_pass = pass != TP_TWO_PASS;
  if (tile_pass) {
    p.tile_stage = c->d_tile_stage;
    p.tile_words = c->d_tile_words;
  }
  p.fq_lines = (pass == TP_FQ && c->want_spans) ? c->d_fqlines.get() : nullptr;
  c->last_spans = false;
  // One build's device work at a time per GPU: each build alone saturates HBM, so builds
  // from different contexts (concurrent goroutines, §8(b) "Threading") run back to back
  // instead of splitting the CUs.  Host staging of other builds still overlaps.
  std::unique_lock<std::mutex> device_lock(device_mutex(c->device));
  // the build's device time runs from its first kernel's start to the end of its last one: a
  // tile pass records its start (and end) in its own dispatch packet (hipExtLaunchKernel), so
  // its start event is ev0; the two-pass build brackets its kernels with stream events
  hipEvent_t k0 = tile_pass ? c->ev0 : c->ek0;
  if (!tile_pass) HIPCHK(hipEventRecord(c->ev0, s), "event");
  static const char *const what[] = {"index launch", "tile pass launch", "FASTA tile pass launch",
                                     "line tile pass launch", "SAM tile pass launch"};  // by TilePass
  HIPCHK(sidx_launch_tiles(pass, &p, d_res, s, k0, c->ek1), what[pass]);
  if (res) res->path = tile_pass ? 1u : 2u;
  HIPCHK(hipEventRecord(c->ev1, s), "event");
  // SHOCKIDX_VERIFY (the GPU test suite): the whole table's contiguity, after the timed kernels
  if (d_rows && verify_rows()) HIPCHK(sidx_launch_verify_rows(d_rows, p.row_base, row_cap, d_res, s), "verify launch");
  HIPCHK(hipMemcpyAsync(c->h_res, d_res, sizeof(DevResult), hipMemcpyDeviceToHost, s), "result copy");
  HIPCHK(hipStreamSynchronize(s), "index sync");
  c->slots_dirty = false;
  if (p.fq_lines) {
    c->last_p = p;
    c->last_spans = true;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  if (res) res->kernel_ms += ms;
  float kms = 0.f;
  (void)hipEventElapsedTime(&kms, k0, c->ek1);
  if (res) res->index_ms = kms;
  *dr = *c->h_res;
  device_lock.unlock();
  // the fix-up queue overflowed (pathological input): redo the build two-pass (the next epoch
  // uses the other first-bad / counter slots, already reset)
  if ((dr->flags & RF_FIXQUEUE) && !general) {
    if (res) res->reruns++;
    return run_index(c, d_data, n, kfmt, d_rows, row_cap, s, dr, res, geom, true, gate);
  }
  return 0;
}

// Translate the device result into (count, status, err).  Returns SHOCKIDX_OK,
// SHOCKIDX_EFORMAT, or a negative code.  FASTA messages read the piece from d_data.
int translate(shockidx_ctx *c, const DevResult &dr, const uint8_t *d_data, hipStream_t s,
              shockidx_result *res) {
  res->count = dr.count;
  res->fixups = dr.fixups;
  res->fix_tiles = dr.fix_tiles;
  res->state_out = dr.state_out;
  res->term_code = dr.code;
  res->flags = dr.flags;
  if (dr.flags & RF_INTERNAL) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: device invariant violated");
  if (dr.flags & RF_HALO) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: slab halo exhausted");
  if (dr.code == ST_OK || dr.code == ST_END || dr.code == ST_ABSENT) {
    res->status = SHOCKIDX_OK;
    return SHOCKIDX_OK;
  }
  if (dr.code == ST_FA_INVALID) {
    return fasta_error_text(res, dr.err_len, [&](char *dst, u64 k) -> int {
      hipError_t e = hipMemcpyAsync(dst, d_data + dr.err_pos, k, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      return e == hipSuccess ? 0 : set_hip(res, e, "error text copy");
    });
  }
  const char *m = status_message(dr.code);
  if (!m) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: unknown device status");
  return set_msg(res, SHOCKIDX_EFORMAT, m);
}

// Index d_data (already in c->d_in or caller memory) into c->d_rows, growing on overflow.
int build_resident(shockidx_ctx *c, const uint8_t *d_data, u64 n, int kind, int fmt, hipStream_t s,
                   shockidx_result *res) {
  int kfmt = 0;
  const int *gate = nullptr;
  if (int rc = resolve_format(c, d_data, n, kind, fmt, s, &kfmt, res, &gate)) return rc;
  res->format = kfmt == F_LINE ? SHOCKIDX_FMT_LINE : kfmt;
  u64 cap = kfmt == F_LINE ? n / 16 + 4096 : n / 32 + 4096;
  for (int attempt = 0; attempt < 3; ++attempt) {
    if (int rc = c->d_rows.ensure(cap, res)) return rc;
    DevResult dr;
    if (int rc = run_index(c, d_data, n, kfmt, c->d_rows, c->d_rows.cap, s, &dr, res, nullptr, false, gate)) return rc;
    if (gate) {
      gate = nullptr;
      if (int rc = respeculate(c, dr, &kfmt, res)) {
        if (rc < 0 || rc == SHOCKIDX_EFORMAT) return rc;
        res->reruns++;
        continue;  // the detected format, ungated
      }
    }
    if (dr.flags & RF_CAPACITY) {  // row capacity overflow: grow to the exact count and rerun
      cap = dr.count;
      res->reruns++;
      continue;
    }
    return translate(c, dr, d_data, s, res);
  }
  return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: row capacity");
}

// The caller's table (free()-able, released by shockidx_free).  Large tables are 2 MiB aligned
// and advised for transparent huge pages: the threaded copy out of the staging buffers then
// faults the fresh memory in 2 MiB pages instead of 4 KiB ones.
uint64_t *alloc_rows_out(size_t bytes) {
  constexpr size_t HUGE = 2u << 20;
  if (bytes < 4 * HUGE) return (uint64_t *)malloc(bytes ? bytes : 16);
  void *p = nullptr;
  if (posix_memalign(&p, HUGE, (bytes + HUGE - 1) & ~(HUGE - 1))) return nullptr;
  (void)madvise(p, (bytes + HUGE - 1) & ~(HUGE - 1), MADV_HUGEPAGE);
  return (uint64_t *)p;
}

// Device rows -> host memory through the pinned staging: the DMA of chunk i + 1 overlaps the
// (threaded) host copy of chunk i.
int rows_to_host(shockidx_ctx *c, const u64 *d_src, size_t bytes, uint8_t *dst, hipStream_t s,
                 Err res) {
  size_t issued = 0, done = 0;
  int i = 0;
  auto issue = [&](int b) -> hipError_t {
    const size_t k = bytes - issued < STAGE_BYTES ? bytes - issued : STAGE_BYTES;
    hipError_t e = hipMemcpyAsync(c->h_stage[b], (const uint8_t *)d_src + issued, k, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(c->stage_ev[b], s);
    issued += k;
    return e;
  };
  hipError_t e = bytes ? issue(0) : hipSuccess;
  while (e == hipSuccess && done < bytes) {
    const size_t k = bytes - done < STAGE_BYTES ? bytes - done : STAGE_BYTES;
    if (issued < bytes) e = issue(i ^ 1);
    if (e == hipSuccess) e = hipEventSynchronize(c->stage_ev[i]);
    if (e != hipSuccess) break;
    c->pool->copy(dst + done, c->h_stage[i], k);
    done += k;
    i ^= 1;
  }
  if (e != hipSuccess) return set_hip(res, e, "rows copy");
  return 0;
}

int fetch_rows(shockidx_ctx *c, u64 count, hipStream_t s, uint64_t **rows, shockidx_result *res) {
  const double t0 = now_ms();
  const size_t bytes = (size_t)count * 16;
  uint64_t *out = alloc_rows_out(bytes);
  if (!out) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
  if (int rc = rows_to_host(c, c->d_rows, bytes, (uint8_t *)out, s, res)) {
    free(out);
    return rc;
  }
  *rows = out;
  res->d2h_ms += now_ms() - t0;
  return 0;
}

// Stage n bytes into c->d_in (from byte `from` on).  `fill(dst, off, len)` produces host bytes
// (memcpy / pread).
template <class Fill>
static int stage_in(shockidx_ctx *c, u64 n, hipStream_t s, Fill fill, shockidx_result *res, u64 from = 0) {
  const double t0 = now_ms();
  if (int rc = c->d_in.ensure(n + 64, res)) return rc;
  u64 off = from;
  int i = 0;
  while (off < n) {
    const size_t k = n - off < STAGE_BYTES ? (size_t)(n - off) : STAGE_BYTES;
    HIPCHK(hipEventSynchronize(c->stage_ev[i]), "stage wait");  // buffer i free again
    if (int rc = fill(c->h_stage[i], off, k)) return rc;
    HIPCHK(hipMemcpyAsync(c->d_in + off, c->h_stage[i], k, hipMemcpyHostToDevice, s), "H2D");
    HIPCHK(hipEventRecord(c->stage_ev[i], s), "stage event");
    off += k;
    i ^= 1;
  }
  HIPCHK(hipStreamSynchronize(s), "H2D sync");
  res->h2d_ms += now_ms() - t0;
  return 0;
}

// Host memory the GPU can DMA from directly (hipHostRegister'ed or hipHostMalloc'ed)
bool host_pinned(const void *p, u64 n) {
  if (!p || !n) return false;
  hipPointerAttribute_t a0, a1;
  const hipError_t e0 = hipPointerGetAttributes(&a0, p);
  (void)hipGetLastError();  // a plain pageable pointer reports an error here
  if (e0 != hipSuccess || a0.type != hipMemoryTypeHost) return false;
  // the last byte too, in the same mapping: a buffer only partly registered (or two adjacent
  // registrations) takes the staging path instead of a DMA that would run past the pinning
  const hipError_t e1 = hipPointerGetAttributes(&a1, (const uint8_t *)p + (n - 1));
  (void)hipGetLastError();
  return e1 == hipSuccess && a1.type == hipMemoryTypeHost && a0.devicePointer && a1.devicePointer &&
         (const uint8_t *)a1.devicePointer - (const uint8_t *)a0.devicePointer == (ptrdiff_t)(n - 1);
}

int stage_host(shockidx_ctx *c, const void *data, u64 n, hipStream_t s, shockidx_result *res) {
  auto fill = [&](uint8_t *dst, u64 off, size_t k) -> int {
    c->pool->copy(dst, (const uint8_t *)data + off, k);
    return 0;
  };
  return stage_in(c, n, s, fill, res);
}

int PreadFill::operator()(uint8_t *dst, u64 off, size_t k) const {
  std::atomic<int> bad{0};
  const int fdl = fd;
  pool->parallel(k, [&, fdl](size_t a, size_t b) {
    size_t got = a;
    while (got < b && !bad.load(std::memory_order_relaxed)) {
      ssize_t r = pread(fdl, dst + got, b - got, (off_t)(off + got));
      if (r < 0) {
        if (errno == EINTR) continue;
        bad.store(errno ? errno : EIO);
        return;
      }
      if (r == 0) { bad.store(-1); return; }
      got += (size_t)r;
    }
  });
  const int e = bad.load();
  if (e == -1) return set_msg(res, SHOCKIDX_EIO, "unexpected end of file");
  if (e) return set_msg(res, SHOCKIDX_EIO, strerror(e));
  return 0;
}

// The page-cache DMA pins a node file's pages until its copy drains.  Bytes a single call may
// keep pinned (several large builds at once could lock that much host RAM):
// SHOCKIDX_PIN_CAP_GIB, else a quarter of the host's memory; past it the rest of the file goes
// through the pinned staging buffers (pread by the copy threads).
static u64 pin_cap() {
  if (const char *e = getenv("SHOCKIDX_PIN_CAP_GIB")) {  // (clamped: a negative or non-numeric value pins nothing)
    const double g = atof(e);
    return g > 0 ? (u64)((g < 1e6 ? g : 1e6) * (double)(1ull << 30)) : 0;
  }
  const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
  return pages > 0 && psz > 0 ? (u64)pages * (u64)psz / 4 : (64ull << 30);
}
// Process-wide pinned host bytes: every page-cache DMA reserves what it pins from one
// budget, pin_cap(), before hipHostRegister and gives it back after unregistering, so concurrent
// builds (a gpuPoolSize of contexts, a multi-GPU group) cannot pin more than the cap together.
// A reservation that fails sends the bytes through the pinned staging buffers instead.
static std::atomic<u64> g_pinned{0};
bool pin_reserve(u64 b) {
  const u64 cap = pin_cap();
  u64 cur = g_pinned.load();
  do {
    if (cur + b > cap) return false;
  } while (!g_pinned.compare_exchange_weak(cur, cur + b));
  return true;
}
void pin_release(u64 b) { g_pinned.fetch_sub(b); }

// Stage the file bytes [off, off + n) into c->d_in.  A file that maps goes to HBM straight out of
// the page cache: mapped read-only, pinned 256 MiB at a time (hipHostRegister), each piece DMA'd
// as soon as it is pinned, everything unpinned once the stream drains (the bytes cross host
// memory once; the fd pipeline does the same per slab).  A file that does not map, or pages
// that do not pin, go (from there on) through the copy threads into the pinned staging.

int stage_fd(shockidx_ctx *c, int fd, u64 off, u64 n, hipStream_t s, shockidx_result *res) {
  u64 done = 0;
  if (n >= (64ull << 20) && !getenv("SHOCKIDX_NO_MMAP_DMA")) {
    if (int rc = c->d_in.ensure(n + 64, res)) return rc;
    const double t0 = now_ms();
    const u64 a0 = off & ~4095ull, lead = off - a0;
    const size_t maplen = (size_t)(((off + n + 4095) & ~4095ull) - a0);
    void *mp = mmap(nullptr, maplen, PROT_READ, MAP_SHARED, fd, (off_t)a0);
    if (mp != MAP_FAILED) {
      uint8_t *map = (uint8_t *)mp;
      constexpr u64 CH = 256ull << 20;
      u64 reg = 0, held = 0;
      hipError_t e = hipSuccess;
      for (u64 mlo = 0; mlo < maplen; mlo += CH) {
        const u64 mhi = maplen - mlo < CH ? maplen : mlo + CH;
        if (!pin_reserve(mhi - mlo)) break;  // over the process-wide pin budget: the rest through the staging buffers
        if (hipHostRegister(map + mlo, (size_t)(mhi - mlo), 0) != hipSuccess) {
          (void)hipGetLastError();
          pin_release(mhi - mlo);
          break;
        }
        ++reg;
        held += mhi - mlo;
        const u64 blo = mlo > lead ? mlo - lead : 0, bhi = mhi - lead < n ? mhi - lead : n;  // file bytes - off
        if (bhi > blo && (e = hipMemcpyAsync(c->d_in + blo, map + lead + blo, bhi - blo, hipMemcpyHostToDevice, s)) != hipSuccess)
          break;
        done = bhi;
      }
      const hipError_t se = hipStreamSynchronize(s);
      for (u64 k = 0; k < reg; ++k) (void)hipHostUnregister(map + k * CH);
      pin_release(held);
      munmap(mp, maplen);
      if (e != hipSuccess) return set_hip(res, e, "page-cache DMA");
      if (se != hipSuccess) return set_hip(res, se, "H2D sync");
      res->h2d_ms += now_ms() - t0;
    }
  }
  if (done >= n) return 0;
  const PreadFill pf{fd, res, c->pool};
  return stage_in(c, n, s, [&](uint8_t *dst, u64 o, size_t k) -> int { return pf(dst, off + o, k); }, res, done);
}

// Device bytes a build may hold: the context's cap (shockidx_ctx_set_dev_cap / SHOCKIDX_DEV_CAP),
// and never more than the device has free plus what this context already holds (its caches are
// freed or reused first).
u64 dev_budget(shockidx_ctx *c) {
  size_t fr = 0, tot = 0;
  u64 avail = ~0ull;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
    const u64 held = workspace_bytes(c);
    avail = (u64)fr + held > (256ull << 20) ? (u64)fr + held - (256ull << 20) : 0;
  } else {
    (void)hipGetLastError();
  }
  return c->dev_cap && c->dev_cap < avail ? c->dev_cap : avail;
}
// what a one-pass build of an n-byte node holds at its peak: the node, its rows (DevBuf::ensure's
// growth included) and the per-tile workspaces
u64 one_pass_bytes(u64 n) { return n + n / 8 + (n / 32) * 16 * 9 / 8 + n / 8 + (64ull << 20); }

hipError_t dev_malloc(void **p, size_t bytes, bool node) {
  if (node && bytes >= (64u << 20) && !getenv("SHOCKIDX_NO_CONTIG")) {
    if (hipExtMallocWithFlags(p, bytes, hipDeviceMallocContiguous) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();  // fragmented: plain memory below
  }
  return hipMalloc(p, bytes);
}

static int hip_alloc(void **p, size_t bytes, bool node) { return (int)dev_malloc(p, bytes, node); }
static void hip_release(void *p) { (void)hipFree(p); }
static const char *hip_errstr(int e) { return hipGetErrorString((hipError_t)e); }
const DevAlloc *hip_allocator() {
  static const DevAlloc a = {hip_alloc, hip_release, hip_errstr};
  return &a;
}

}  // namespace sidx_host
