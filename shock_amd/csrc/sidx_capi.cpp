// sidx_capi.cpp -- the C ABI declared in include/shockidx.h: the context's lifecycle, the build
// entry points (device, host memory, file descriptor), Create and the .idx writer with the
// reference's temp-file + rename protocol (shock-server/node/file/index/record.go:35-41,65-87),
// device memory, the multi-GPU slab and communicator entry points, format detection.  The work
// is in sidx_build.cpp (one index build, staging), sidx_pipeline.cpp and sidx_walks.cpp (the slab walks);
// chunkrecord, subset and filter entry points have files of their own.  No index computation
// happens on the host: without a usable GPU every entry point fails with SHOCKIDX_EHIP.
#include <errno.h>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <random>
#include <string>
#include <thread>

#include <rccl/rccl.h>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_subset.hpp"
#include "sidx_launch.hpp"
#include "sidx_slabwalk.hpp"
#include "sidx_walk.hpp"

using namespace sidx;
using namespace sidx_host;

namespace {

// "2147483648", "2G", "512M", "64K" (binary units); anything unparsable is 0 (no cap)
u64 parse_bytes(const char *v) {
  char *end = nullptr;
  const double x = strtod(v, &end);
  if (!(x > 0) || end == v) return 0;
  const double m = (*end == 'G' || *end == 'g') ? 1073741824.0 : (*end == 'M' || *end == 'm') ? 1048576.0
                   : (*end == 'K' || *end == 'k') ? 1024.0 : 1.0;
  return x * m < 1.8e19 ? (u64)(x * m) : ~0ull;
}

constexpr u64 PIN_PIECE = 1ull << 30;

// record.go:35 tmpFilePath := fmt.Sprintf("%s/temp/%d%d.idx", conf.PATH_DATA, rand.Int(), rand.Int())
// (the caller passes PATH_DATA/temp as tmpdir)
std::string temp_idx_path(const char *tmpdir) {
  static std::atomic<unsigned long long> salt{0};
  std::mt19937_64 rng((unsigned long long)now_ms() * 1000003ull ^ (unsigned long long)getpid() ^ (salt++ << 20));
  return std::string(tmpdir) + "/" + std::to_string(rng() >> 1) + std::to_string(rng() >> 1) + ".idx";
}

}  // namespace

extern "C" {

int shockidx_abi_version(void) { return SHOCKIDX_ABI_VERSION; }

const char *shockidx_strerror(int code) {
  switch (code) {
    case SHOCKIDX_OK: return "ok";
    case SHOCKIDX_EFORMAT: return "format error";
    case SHOCKIDX_EINVAL: return "invalid argument";
    case SHOCKIDX_EHIP: return "HIP runtime error";
    case SHOCKIDX_ENOMEM: return "out of memory";
    case SHOCKIDX_EIO: return "I/O error";
    case SHOCKIDX_EINTERNAL: return "internal error";
    case SHOCKIDX_ESPACE: return "output capacity too small";
    default: return "unknown";
  }
}

void shockidx_free(void *p) { free(p); }

int shockidx_host_register(shockidx_ctx *c, void *p, uint64_t n) {
  const Err res;  // (the text is discarded: the code is what the caller gets)
  if (!c || !p || !n) return SHOCKIDX_EINVAL;
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  HIPCHK(hipHostRegister(p, n, hipHostRegisterDefault), "hipHostRegister");
  return SHOCKIDX_OK;
}

int shockidx_host_unregister(shockidx_ctx *c, void *p) {
  const Err res;  // (the text is discarded: the code is what the caller gets)
  if (!c || !p) return SHOCKIDX_EINVAL;
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  HIPCHK(hipHostUnregister(p), "hipHostUnregister");
  return SHOCKIDX_OK;
}

int shockidx_ctx_create(int device, shockidx_ctx **out) {
  const Err res;  // (the text is discarded: the code is what the caller gets)
  if (!out) return SHOCKIDX_EINVAL;
  *out = nullptr;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
  if (device < 0 || device >= ndev) return SHOCKIDX_EINVAL;
  HIPCHK(hipSetDevice(device), "hipSetDevice");
  shockidx_ctx *c = new shockidx_ctx();
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&c->ev0);
  if (e == hipSuccess) e = hipEventCreate(&c->ev1);
  if (e == hipSuccess) e = hipEventCreate(&c->ek0);
  if (e == hipSuccess) e = hipEventCreate(&c->ek1);
  for (int i = 0; i < NSTAGE && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->stage_ev[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&c->d_small, SMALL_BYTES);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_small, 0, SMALL_BYTES, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_small + SMALL_BADKEY, 0xFF, 16, c->stream);  // both first-bad slots
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) {
    // persistent grids: one wave of co-resident workgroups over the CUs
    int cus = 0;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    int pp = sidx_tiles_blocks_per_cu();
    if (const char *w = getenv("SHOCKIDX_TILES_PER_CU")) pp = atoi(w) < pp ? atoi(w) : pp;  // tuning knob
    c->tiles_grid = (u32)(cus * (pp < 1 ? 1 : pp));
    const int vb = sidx_cr_verify_blocks_per_cu();
    c->cr_grid = (u32)(cus * (vb < 1 ? 1 : vb));
  }
  for (int i = 0; i < NSTAGE && e == hipSuccess; ++i) e = hipHostMalloc(&c->h_stage[i], STAGE_BYTES, 0);
  if (e == hipSuccess) e = hipHostMalloc(&c->h_res, sizeof(DevResult), 0);
  if (e == hipSuccess) e = hipHostMalloc(&c->h_det, 64, 0);
  if (e == hipSuccess) {
    const unsigned hw = std::thread::hardware_concurrency();
    // 16 (a GPU's share of the host's cores on an 8-GPU MI355X node): the page-cached fd path
    // (pread into the pinned staging) ran 32.6 GiB/s with 8 threads, 38.2 with 16
    int nt = getenv("SHOCKIDX_COPY_THREADS") ? atoi(getenv("SHOCKIDX_COPY_THREADS")) : (int)(hw / 2 < 16 ? hw / 2 : 16);
    c->pool = new CopyPool(nt < 1 ? 1 : nt);
  }
  if (const char *cap = getenv("SHOCKIDX_WORKSPACE_CAP")) c->ws_cap = strtoull(cap, nullptr, 10);
  if (const char *cap = getenv("SHOCKIDX_DEV_CAP")) c->dev_cap = parse_bytes(cap);
  if (e != hipSuccess) {
    shockidx_ctx_destroy(c);
    return SHOCKIDX_EHIP;
  }
  *out = c;
  return SHOCKIDX_OK;
}

int shockidx_ctx_set_dev_cap(shockidx_ctx *c, uint64_t bytes) {
  if (!c) return SHOCKIDX_EINVAL;
  c->dev_cap = bytes;
  return SHOCKIDX_OK;
}

int shockidx_ctx_trim(shockidx_ctx *c, uint64_t keep_bytes) {
  if (!c) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  trim_workspace(c, keep_bytes);
  return SHOCKIDX_OK;
}

uint64_t shockidx_ctx_workspace_bytes(shockidx_ctx *c) { return c ? workspace_bytes(c) : 0; }

void shockidx_ctx_destroy(shockidx_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->bufs.drop_all();
  (void)hipFree(c->d_small);
  (void)hipFree(c->d_timing);
  for (int i = 0; i < NSTAGE; ++i) {
    if (c->h_stage[i]) (void)hipHostFree(c->h_stage[i]);
    if (c->stage_ev[i]) (void)hipEventDestroy(c->stage_ev[i]);
  }
  if (c->h_res) (void)hipHostFree(c->h_res);
  if (c->h_det) (void)hipHostFree(c->h_det);
  delete c->pool;
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ek0) (void)hipEventDestroy(c->ek0);
  if (c->ek1) (void)hipEventDestroy(c->ek1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->s_copy) (void)hipStreamDestroy(c->s_copy);
  for (int i = 0; i < 2; ++i)
    if (c->h_rows[i]) (void)hipHostFree(c->h_rows[i]);
  delete c;
}

int shockidx_build_device(shockidx_ctx *c, const void *d_data, uint64_t n, int kind, int fmt,
                          void *d_rows, uint64_t row_cap, void *stream, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || (!d_data && n) || ((uintptr_t)d_data & 15)) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const uint8_t *dd = (const uint8_t *)d_data;
  int kfmt = 0;
  const int *gate = nullptr;
  if (int rc = resolve_format(c, dd, n, kind, fmt, s, &kfmt, res, &gate)) return rc;
  res->format = kfmt == F_LINE ? SHOCKIDX_FMT_LINE : kfmt;
  DevResult dr;
  if (int rc = run_index(c, dd, n, kfmt, (u64 *)d_rows, row_cap, s, &dr, res, nullptr, false, gate)) return rc;
  if (gate) {
    if (int rr = respeculate(c, dr, &kfmt, res)) {
      if (rr < 0 || rr == SHOCKIDX_EFORMAT) return rr;
      res->reruns++;
      if (int rc = run_index(c, dd, n, kfmt, (u64 *)d_rows, row_cap, s, &dr, res)) return rc;
    }
  }
  int rc = translate(c, dr, dd, s, res);
  if (rc >= 0 && (dr.flags & RF_CAPACITY)) rc = set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  res->count = dr.count;
  res->total_ms = now_ms() - t0;
  return rc;
}

int shockidx_build_host(shockidx_ctx *c, const void *data, uint64_t n, int kind, int fmt,
                        uint64_t **rows, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !rows || (!data && n)) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  const double t0 = now_ms();
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  bool piped = false;
  if (int rc = build_host_pipelined(c, data, n, kind, fmt, rows, res, &piped); piped) return rc;
  if (host_pinned(data, n)) {  // registered / hipHostMalloc'ed: DMA straight from the caller's pages
    const double th = now_ms();
    if (int rc = c->d_in.ensure(n + 64, res)) return rc;
    for (u64 off = 0; off < n; off += PIN_PIECE) {
      const u64 k = n - off < PIN_PIECE ? n - off : PIN_PIECE;
      HIPCHK(hipMemcpyAsync(c->d_in + off, (const uint8_t *)data + off, k, hipMemcpyHostToDevice, s), "H2D");
    }
    HIPCHK(hipStreamSynchronize(s), "H2D sync");
    res->h2d_ms += now_ms() - th;
  } else if (int rc = stage_host(c, data, n, s, res)) {
    return rc;
  }
  int rc = build_resident(c, c->d_in, n, kind, fmt, s, res);
  if (rc < 0) return rc;
  if (int rc2 = fetch_rows(c, res->count, s, rows, res)) return rc2;
  res->total_ms = now_ms() - t0;
  return rc;
}

int shockidx_build_fd(shockidx_ctx *c, int fd, uint64_t n, int kind, int fmt, uint64_t **rows,
                      shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !rows || fd < 0) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  const double t0 = now_ms();
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  {
    TableSink sink(n);
    bool piped = false, fell = false;
    int rc = build_fd_pipelined(c, fd, n, kind, fmt, sink, res, &piped, &fell);
    if (piped) {
      if (rc < 0) return rc;
      if (!fell) {  // the table as it arrived (trimmed to the rows)
        uint8_t *t = sink.out;
        sink.out = nullptr;
        if (!t) t = (uint8_t *)malloc(16);
        *rows = (uint64_t *)t;
        if (!*rows) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
        res->total_ms = now_ms() - t0;
        return rc;
      }
      if (int rc2 = fetch_rows(c, res->count, s, rows, res)) return rc2;
      res->total_ms = now_ms() - t0;
      return rc;
    }
  }
  if (int rc = stage_fd(c, fd, 0, n, s, res)) return rc;
  int rc = build_resident(c, c->d_in, n, kind, fmt, s, res);
  if (rc < 0) return rc;
  if (int rc2 = fetch_rows(c, res->count, s, rows, res)) return rc2;
  res->total_ms = now_ms() - t0;
  return rc;
}

int shockidx_write_idx(const uint64_t *rows, uint64_t count, const char *tmpdir, const char *outpath,
                       char *err, size_t errlen) {
  auto fail = [&](const char *what) {
    if (err && errlen) snprintf(err, errlen, "%s: %s", what, strerror(errno));
    return SHOCKIDX_EIO;
  };
  if (!tmpdir || !outpath || (!rows && count)) return SHOCKIDX_EINVAL;
  std::string tmp = temp_idx_path(tmpdir);
  int fd = open(tmp.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0666);
  if (fd < 0) return fail("create");
  const uint8_t *p = (const uint8_t *)rows;
  size_t left = (size_t)count * 16;
  while (left) {  // rows are {u64 off, u64 len} little-endian in memory (record.go:74-75)
    ssize_t w = write(fd, p, left > (1u << 30) ? (1u << 30) : left);
    if (w < 0) {
      if (errno == EINTR) continue;
      int e = errno;
      close(fd);
      unlink(tmp.c_str());
      errno = e;
      return fail("write");
    }
    p += w;
    left -= (size_t)w;
  }
  if (close(fd) != 0) { unlink(tmp.c_str()); return fail("close"); }
  if (rename(tmp.c_str(), outpath) != 0) {  // record.go:87
    int e = errno;
    unlink(tmp.c_str());
    errno = e;
    return fail("rename");
  }
  return SHOCKIDX_OK;
}

int shockidx_create(shockidx_ctx *c, int fd, uint64_t n, int kind, const char *tmpdir, const char *outpath,
                    shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  if (c && fd >= 0 && tmpdir && outpath && n >= 2 * PIPE_SLAB) {
    // the slab pipeline writes each slab's rows into the temp file while later slabs are read
    reset_result(res);
    const double t0 = now_ms();
    TrimGuard trim{c};
    HIPCHK(hipSetDevice(c->device), "hipSetDevice");
    FileSink sink;
    const std::string tpath = temp_idx_path(tmpdir);
    sink.fd = open(tpath.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0666);
    if (sink.fd < 0) {
      return set_msg(res, SHOCKIDX_EIO, std::string("create: ") + strerror(errno));
    }
    bool piped = false, fell = false;
    int rc = build_fd_pipelined(c, fd, n, kind, SHOCKIDX_FMT_AUTO, sink, res, &piped, &fell);
    if (piped && !fell && rc == SHOCKIDX_OK) {
      const int ce = close(sink.fd);
      if (ce != 0 || rename(tpath.c_str(), outpath) != 0) {  // record.go:87
        const int e = errno;
        unlink(tpath.c_str());
        return set_msg(res, SHOCKIDX_EIO, std::string(ce != 0 ? "close: " : "rename: ") + strerror(e));
      }
      res->total_ms = now_ms() - t0;
      return SHOCKIDX_OK;
    }
    close(sink.fd);
    unlink(tpath.c_str());
    if (piped) {  // fell back (or failed): the one-pass result, written like the plain path
      if (rc != SHOCKIDX_OK) return rc;
      uint64_t *rows = nullptr;
      if (int rc2 = fetch_rows(c, res->count, c->stream, &rows, res)) return rc2;
      int w = shockidx_write_idx(rows, res->count, tmpdir, outpath, res->err, sizeof res->err);
      free(rows);
      if (w != SHOCKIDX_OK) return set_msg(res, w, res->err);
      res->total_ms = now_ms() - t0;
      return SHOCKIDX_OK;
    }
  }
  uint64_t *rows = nullptr;
  int rc = shockidx_build_fd(c, fd, n, kind, SHOCKIDX_FMT_AUTO, &rows, res);
  if (rc != SHOCKIDX_OK) {
    free(rows);
    return rc;
  }
  const double t0 = now_ms();
  int w = shockidx_write_idx(rows, res->count, tmpdir, outpath, res->err, sizeof res->err);
  free(rows);
  if (w != SHOCKIDX_OK) return set_msg(res, w, res->err);
  res->total_ms += now_ms() - t0;
  return SHOCKIDX_OK;
}

// CreateColumnIndex's file protocol (column.go:34-40,109-129).  Within the device budget: the
// whole-node build, its table written in one piece.  Else the slab walk, each slab's rows written
// at 16 * row as they arrive; whatever ends the walk early -- the missing-column line may sit in
// the last slab, after rows were written -- takes the temp file with it.
int shockidx_column_create(shockidx_ctx *c, int fd, uint64_t n, int column, const char *tmpdir, const char *outpath,
                           shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  res->format = SHOCKIDX_FMT_LINE;
  if (!c || fd < 0 || column < 1 || !tmpdir || !outpath) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  if (column_whole_bytes(n) <= dev_budget(c)) {
    uint64_t *rows = nullptr;
    const int rc = shockidx_column_fd(c, fd, n, column, &rows, res);
    if (rc != SHOCKIDX_OK) {
      free(rows);
      return rc;
    }
    const double t0 = now_ms();
    const int w = shockidx_write_idx(rows, res->count, tmpdir, outpath, res->err, sizeof res->err);
    free(rows);
    if (w != SHOCKIDX_OK) return set_msg(res, w, res->err);
    res->total_ms += now_ms() - t0;
    return SHOCKIDX_OK;
  }
  TrimGuard trim{c};
  FileSink sink;
  const std::string tpath = temp_idx_path(tmpdir);
  sink.fd = open(tpath.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0666);
  if (sink.fd < 0) return set_msg(res, SHOCKIDX_EIO, std::string("create: ") + strerror(errno));
  const int rc = column_fd_walk(c, fd, n, (u32)column, 0, 0, sink, res);
  const int ce = close(sink.fd);
  if (rc != SHOCKIDX_OK) {
    unlink(tpath.c_str());
    return rc;
  }
  if (ce != 0 || rename(tpath.c_str(), outpath) != 0) {  // column.go:127
    const int e = errno;
    unlink(tpath.c_str());
    return set_msg(res, SHOCKIDX_EIO, std::string(ce != 0 ? "close: " : "rename: ") + strerror(e));
  }
  return SHOCKIDX_OK;
}

// ---- the subset indexes from files (index/subset.go:36-303) -------------------------------------
namespace {

// Today's whole build over the two uploaded files: the id text in c->d_in, the parent index in
// c->d_spar, the rows in c->d_cola and the runs in c->d_sruns (shockidx_subset_index keeps its line
// ends in c->d_rows); the tables to the sinks.  A table too short for the ids is grown to the
// count the build reports and the build run again.
int subset_whole(shockidx_ctx *c, int ids_fd, u64 n, int parent_fd, u64 parent_bytes, i64 ilength, bool want_runs,
                 SubsetSinks sinks, shockidx_subset_result *res) {
  hipStream_t s = c->stream;
  const u64 parent_count = parent_bytes / 16;
  shockidx_result r1;
  reset_result(&r1);
  if (int rc = stage_fd(c, ids_fd, 0, n, s, &r1)) return forward_error(res, r1, rc);
  if (int rc = c->d_spar.ensure(16 * parent_count + 16, res)) return rc;
  if (int rc = walk_prereqs(c, res)) return rc;
  if (int rc = file_to_device(c, parent_fd, 0, 16 * parent_count, c->d_spar, "", "unexpected end of file", "parent copy", res))
    return rc;
  u64 rows_cap = n / 8 + 4096, runs_cap = want_runs ? rows_cap : 0;
  int rc = 0;
  for (int attempt = 0;; ++attempt) {
    if (int e = c->d_cola.ensure(16 * rows_cap, res)) return e;
    if (want_runs)
      if (int e = c->d_sruns.ensure(16 * runs_cap, res)) return e;
    rc = shockidx_subset_index(c, c->d_in, n, c->d_spar, parent_count, ilength, c->d_cola, rows_cap,
                               want_runs ? (void *)c->d_sruns : nullptr, runs_cap, res);
    if (rc != SHOCKIDX_ESPACE || attempt == 2) break;
    if (res->count > rows_cap) rows_cap = res->count;
    if (want_runs && res->runs + 1 > runs_cap) runs_cap = res->runs + 1;
  }
  if (rc != SHOCKIDX_OK && rc != SHOCKIDX_EFORMAT) return rc;
  const shockidx_subset_result keep = *res;
  if (int e = drain_rows(c, c->d_cola.as<u64>(), keep.count, 0, *sinks.rows, nullptr, nullptr, res)) return e;
  if (want_runs)
    if (int e = drain_rows(c, c->d_sruns.as<u64>(), keep.runs, 0, *sinks.runs, nullptr, nullptr, res)) return e;
  *res = keep;
  return rc;
}

}  // namespace

int shockidx_subset_fd_walk(shockidx_ctx *c, int ids_fd, uint64_t ids_size, int parent_fd, uint64_t parent_bytes,
                            int64_t ilength, int want_runs, uint64_t ids_slab_bytes, uint64_t parent_slab_rows,
                            uint64_t **rows, uint64_t **runs, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || ids_fd < 0 || parent_fd < 0 || !rows || (want_runs && !runs))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  if (runs) *runs = nullptr;
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  TableSink srows(ids_size), sruns(want_runs ? ids_size : 0);
  if (!srows.out || !sruns.out) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
  const int rc = subset_fd_walk(c, ids_fd, ids_size, parent_fd, parent_bytes, ilength, want_runs != 0, ids_slab_bytes,
                                parent_slab_rows, SubsetSinks{&srows, &sruns}, res);
  if (rc != SHOCKIDX_OK && rc != SHOCKIDX_EFORMAT) return rc;
  *rows = (uint64_t *)srows.out;
  srows.out = nullptr;
  if (want_runs) {
    *runs = (uint64_t *)sruns.out;
    sruns.out = nullptr;
  }
  return rc;
}

// CreateSubsetNodeIndexes' file protocol (subset.go:136-158,274-297), CreateSubsetIndex's with
// cofile == NULL (:36-128).  Within the device budget the whole build over the uploaded files,
// else the walk, which writes both tables at 16 * row as its calls deliver them.  Whatever ends the
// build early takes both temp files with it (the reference leaves them in conf.PATH_DATA/temp).
int shockidx_subset_create(shockidx_ctx *c, int ids_fd, uint64_t ids_size, int parent_fd, uint64_t parent_bytes,
                           int64_t ilength, const char *tmpdir, const char *cofile, const char *ofile,
                           shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || ids_fd < 0 || parent_fd < 0 || !tmpdir || !ofile) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  TrimGuard trim{c};
  const bool want_runs = cofile != nullptr;
  FileSink srows, sruns;
  const std::string opath = temp_idx_path(tmpdir), copath = want_runs ? temp_idx_path(tmpdir) : std::string();
  srows.fd = open(opath.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0666);
  if (srows.fd < 0) return set_msg(res, SHOCKIDX_EIO, std::string("create: ") + strerror(errno));
  if (want_runs) {
    sruns.fd = open(copath.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0666);
    if (sruns.fd < 0) {
      const int e = errno;
      close(srows.fd);
      unlink(opath.c_str());
      return set_msg(res, SHOCKIDX_EIO, std::string("create: ") + strerror(e));
    }
  }
  int rc;
  if (subset_whole_bytes(ids_size, parent_bytes) <= dev_budget(c)) {
    memset(&c->subset_stats, 0, sizeof c->subset_stats);
    rc = subset_whole(c, ids_fd, ids_size, parent_fd, parent_bytes, ilength, want_runs, SubsetSinks{&srows, &sruns}, res);
    c->subset_stats.ids_bytes = ids_size;
    c->subset_stats.parent_bytes = parent_bytes / 16 * 16;
    c->subset_stats.held_bytes = workspace_bytes(c);
  } else {
    rc = subset_fd_walk(c, ids_fd, ids_size, parent_fd, parent_bytes, ilength, want_runs, 0, 0,
                        SubsetSinks{&srows, &sruns}, res);
  }
  int ce = close(srows.fd);
  if (want_runs && close(sruns.fd) != 0) ce = -1;
  const int e0 = errno;
  auto drop = [&]() {
    unlink(opath.c_str());
    if (want_runs) unlink(copath.c_str());
  };
  if (rc != SHOCKIDX_OK) {
    drop();
    if (rc == SHOCKIDX_EFORMAT && !want_runs) res->count = res->size = ~0ull;  // (-1, -1, err): subset.go:36-128
    if (!want_runs) res->runs = 0;
    return rc;
  }
  if (ce != 0) {
    drop();
    return set_msg(res, SHOCKIDX_EIO, std::string("close: ") + strerror(e0));
  }
  if (want_runs && rename(copath.c_str(), cofile) != 0) {  // :293
    const int e = errno;
    drop();
    return set_msg(res, SHOCKIDX_EIO, std::string("rename: ") + strerror(e));
  }
  if (rename(opath.c_str(), ofile) != 0) {  // :297
    const int e = errno;
    drop();
    if (want_runs) unlink(cofile);
    return set_msg(res, SHOCKIDX_EIO, std::string("rename: ") + strerror(e));
  }
  if (!want_runs) res->runs = 0;
  return SHOCKIDX_OK;
}

int shockidx_subset_last_stats(const shockidx_ctx *c, shockidx_subset_stats *out) {
  if (!c || !out) return SHOCKIDX_EINVAL;
  *out = c->subset_stats;
  return SHOCKIDX_OK;
}

int shockidx_dev_alloc(shockidx_ctx *c, uint64_t bytes, void **d_ptr) {
  if (!c || !d_ptr) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  return dev_malloc(d_ptr, bytes ? bytes : 16, false) == hipSuccess ? SHOCKIDX_OK : SHOCKIDX_ENOMEM;
}

int shockidx_dev_alloc_node(shockidx_ctx *c, uint64_t bytes, void **d_ptr) {
  if (!c || !d_ptr) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  return dev_malloc(d_ptr, bytes ? bytes : 16, true) == hipSuccess ? SHOCKIDX_OK : SHOCKIDX_ENOMEM;
}

int shockidx_dev_free(shockidx_ctx *c, void *d_ptr) {
  if (!c) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  return hipFree(d_ptr) == hipSuccess ? SHOCKIDX_OK : SHOCKIDX_EHIP;
}

// Both copies run on the context's stream and are waited for: the context streams are
// non-blocking, so a null-stream hipMemcpy is not ordered with their kernels, and a pageable
// host-to-device hipMemcpy may return before its DMA has landed -- a build launched right after
// on another context's stream could read the old bytes.
int shockidx_memcpy_h2d(shockidx_ctx *c, void *d_dst, const void *src, uint64_t bytes) {
  if (!c) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  if (hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return SHOCKIDX_EHIP;
  return hipStreamSynchronize(c->stream) == hipSuccess ? SHOCKIDX_OK : SHOCKIDX_EHIP;
}

int shockidx_memcpy_d2h(shockidx_ctx *c, void *dst, const void *d_src, uint64_t bytes) {
  if (!c) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  if (hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return SHOCKIDX_EHIP;
  return hipStreamSynchronize(c->stream) == hipSuccess ? SHOCKIDX_OK : SHOCKIDX_EHIP;
}

int shockidx_memset(shockidx_ctx *c, void *d_dst, int value, uint64_t bytes) {
  if (!c) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  if (hipMemsetAsync(d_dst, value, bytes, c->stream) != hipSuccess) return SHOCKIDX_EHIP;
  return hipStreamSynchronize(c->stream) == hipSuccess ? SHOCKIDX_OK : SHOCKIDX_EHIP;
}

int shockidx_sync(shockidx_ctx *c) {
  if (!c) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  return hipDeviceSynchronize() == hipSuccess ? SHOCKIDX_OK : SHOCKIDX_EHIP;
}

void *shockidx_stream(shockidx_ctx *c) { return c ? (void *)c->stream : nullptr; }

// Diagnostic (not in the public header): copy the per-workgroup phase cycle sums of the
// last build made with SHOCKIDX_TIMING set into out[9 * nwg].
int shockidx_debug_timing(shockidx_ctx *c, uint64_t *out, uint32_t nwg) {
  if (!c || !c->d_timing || !out || nwg > 65536) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  if (hipDeviceSynchronize() != hipSuccess) return SHOCKIDX_EHIP;
  return hipMemcpy(out, c->d_timing, 9 * 8 * (size_t)nwg, hipMemcpyDeviceToHost) == hipSuccess ? SHOCKIDX_OK
                                                                                              : SHOCKIDX_EHIP;
}

int shockidx_debug_tiles_grid(shockidx_ctx *c) { return c ? (int)c->tiles_grid : 0; }

// Diagnostic (not in the public header): run every tile pass of this context on at most g
// workgroups, so a test reaches every edge of the claim plan (sidx_claim.hpp) with a few MiB.
// Only before the context's first build (the workspace is sized by the grid); g in 1..the grid.
int shockidx_debug_set_tiles_grid(shockidx_ctx *c, int g) {
  if (!c || c->epoch != 0 || g < 1 || (u32)g > c->tiles_grid) return SHOCKIDX_EINVAL;
  c->tiles_grid = c->grid_cap = (u32)g;
  return SHOCKIDX_OK;
}

// Diagnostic (not in the public header): test hooks of the context (shockidx_ctx::inject);
// returns the previous flags.  The next build that grows the status arrays takes bits 0-1.
int shockidx_debug_inject(shockidx_ctx *c, uint32_t flags) {
  if (!c) return SHOCKIDX_EINVAL;
  const int old = (int)c->inject;
  c->inject = flags;
  return old;
}

int shockidx_slab_guess(shockidx_ctx *c, const shockidx_slab *sl, int fmt, uint64_t *guess) {
  const Err res;  // (the text is discarded: the code is what the caller gets)
  if (!c || !sl || !guess) return SHOCKIDX_EINVAL;
  if (sl->is_first) { *guess = 0; return SHOCKIDX_OK; }
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  u64 *d_out = (u64 *)(c->d_small + SMALL_DETECT + 32);
  HIPCHK(sidx_launch_slab_guess((const uint8_t *)sl->d_data, sl->n, sl->front, fmt, d_out, s), "guess launch");
  HIPCHK(hipMemcpyAsync(c->h_det + 2, d_out, 8, hipMemcpyDeviceToHost, s), "guess copy");
  HIPCHK(hipStreamSynchronize(s), "guess sync");
  memcpy(guess, c->h_det + 2, 8);
  return SHOCKIDX_OK;
}

int shockidx_slab_index(shockidx_ctx *c, const shockidx_slab *sl, int fmt, uint64_t state_in, void *d_rows,
                        uint64_t row_cap, void *d_summary, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  // an empty slab owns no bytes: its pointer may sit at an unaligned file end (tiny files
  // cut into more slabs than 16-byte chunks); nothing is loaded through it
  const bool empty = sl && sl->n == 0 && !sl->is_first;
  if (!c || !sl || !d_summary || (!empty && ((uintptr_t)sl->d_data & 15)) || sl->end < sl->n ||
      (!sl->is_first && sl->n > 0 && sl->front < 16))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid slab");
  if (fmt < SHOCKIDX_FMT_FASTA || fmt > SHOCKIDX_FMT_LINE) return set_msg(res, SHOCKIDX_EINVAL, "invalid format");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  SlabGeom g;
  g.n = sl->n;
  g.end = empty ? 0 : sl->end;
  g.front = (sl->is_first || empty) ? 0 : sl->front;
  g.base = sl->base;
  g.state_in = state_in;
  g.row_base = sl->is_first ? 0 : 1;  // record 0 belongs to the first slab
  g.eof = sl->is_last;
  g.file_start = sl->is_first;
  g.d_summary = d_summary;
  g.seq = sl->seq;
  res->format = fmt;
  DevResult dr;
  if (int rc = run_index(c, (const uint8_t *)sl->d_data, sl->n, fmt, (u64 *)d_rows, row_cap, c->stream, &dr, res, &g))
    return rc;
  res->count = dr.count;
  res->state_out = dr.state_out;
  res->term_code = dr.code;
  res->flags = dr.flags;
  res->fixups = dr.fixups;
  res->total_ms = now_ms() - t0;
  if (dr.flags & RF_INTERNAL) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: device invariant violated");
  return SHOCKIDX_OK;
}

int shockidx_slab_combine(shockidx_ctx *c, const void *d_all, int world, int rank, int fmt,
                          const uint32_t *expect_seq, shockidx_slab_plan *plan) {
  const Err res;  // (the text is discarded: the code is what the caller gets)
  if (!c || !d_all || !plan || world < 1 || world > 32 || rank < 0 || rank >= world) return SHOCKIDX_EINVAL;
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  void *d_plan = c->d_small + SMALL_RESULT + sizeof(DevResult);
  static_assert(SMALL_RESULT + sizeof(DevResult) + sizeof(SlabPlan) <= SMALL_DETECT, "small layout");
  HIPCHK(sidx_launch_slab_combine(d_all, world, rank, fmt, expect_seq, d_plan, s), "combine launch");
  HIPCHK(hipMemcpyAsync(c->h_res, d_plan, sizeof(SlabPlan), hipMemcpyDeviceToHost, s), "plan copy");
  HIPCHK(hipStreamSynchronize(s), "combine sync");
  static_assert(sizeof(SlabPlan) == sizeof(shockidx_slab_plan), "plan layout");
  memcpy(plan, c->h_res, sizeof(SlabPlan));
  return SHOCKIDX_OK;
}

struct shockidx_comm {
  ncclComm_t comm;
  hipStream_t stream;
  int device;
};

int shockidx_comm_unique_id(void *id128) {
  static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id size");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return SHOCKIDX_EHIP;
  memcpy(id128, &id, sizeof id);
  return SHOCKIDX_OK;
}

int shockidx_comm_init(shockidx_ctx *c, int world, int rank, const void *id128, shockidx_comm **out) {
  if (!c || !id128 || !out) return SHOCKIDX_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess) return SHOCKIDX_EHIP;
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  shockidx_comm *m = new shockidx_comm();
  m->stream = c->stream;
  m->device = c->device;
  if (ncclCommInitRank(&m->comm, world, id, rank) != ncclSuccess) {
    delete m;
    return SHOCKIDX_EHIP;
  }
  *out = m;
  return SHOCKIDX_OK;
}

int shockidx_comm_allgather(shockidx_comm *m, const void *d_send, void *d_recv, uint64_t bytes) {
  if (!m) return SHOCKIDX_EINVAL;
  if (hipSetDevice(m->device) != hipSuccess) return SHOCKIDX_EHIP;
  if (ncclAllGather(d_send, d_recv, bytes, ncclUint8, m->comm, m->stream) != ncclSuccess) return SHOCKIDX_EHIP;
  return SHOCKIDX_OK;
}

int shockidx_comm_count(const shockidx_comm *m, int *nranks) {
  if (!m || !nranks) return SHOCKIDX_EINVAL;
  int n = 0;
  if (ncclCommCount(m->comm, &n) != ncclSuccess) return SHOCKIDX_EHIP;
  *nranks = n;
  return SHOCKIDX_OK;
}

int shockidx_comm_destroy(shockidx_comm *m) {
  if (!m) return SHOCKIDX_EINVAL;
  ncclCommDestroy(m->comm);
  delete m;
  return SHOCKIDX_OK;
}

int shockidx_detect(shockidx_ctx *c, const void *data, uint64_t n, int *fmt, int *mask) {
  const Err res;  // (the text is discarded: the code is what the caller gets)
  if (!c || (!data && n) || !fmt) return SHOCKIDX_EINVAL;
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const u64 m = n < 32768 ? n : 32768;
  if (int rc = c->d_in.ensure(m + 64, res)) return rc;
  if (m) {
    memcpy(c->h_stage[0], data, m);
    HIPCHK(hipMemcpyAsync(c->d_in, c->h_stage[0], m, hipMemcpyHostToDevice, s), "H2D");
  }
  int *d_det = (int *)(c->d_small + SMALL_DETECT);
  HIPCHK(sidx_launch_detect(c->d_in, m, d_det, s), "detect launch");
  HIPCHK(hipMemcpyAsync(c->h_det, d_det, 2 * sizeof(int), hipMemcpyDeviceToHost, s), "detect copy");
  HIPCHK(hipStreamSynchronize(s), "detect sync");
  *fmt = c->h_det[0];
  if (mask) *mask = c->h_det[1];
  return SHOCKIDX_OK;
}

}  // extern "C"
