// sidx_host.hpp -- the host side of libshockidx as its translation units see each other: the
// context and its device caches (sidx_devbuf.hpp), the error helpers, and the functions of
// sidx_build.cpp (workspaces, one index pass, staging, copy-out), sidx_pipeline.cpp (the record
// slab pipelines) and sidx_walks.cpp (the column, subset and chunkrecord walks) that the entry
// points call.  What those two share among themselves is in sidx_walk.hpp.
// Internal: not part of the C ABI (include/shockidx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_devbuf.hpp"

namespace sidx {
struct ChunkWalkDev;  // sidx_chunkwalk.hpp
struct FiltWalkDev;   // sidx_filtwalk.hpp
}

namespace sidx_host {

constexpr size_t STAGE_BYTES = 64ull << 20;  // pinned staging chunk
constexpr int NSTAGE = 2;
// c->d_small: badkey slots at +0/+8, counter slots at +64/+80
constexpr size_t SMALL_BADKEY = 0, SMALL_COUNTERS = 64, SMALL_RESULT = 128, SMALL_DETECT = 320, SMALL_CHUNK = 384,
                 SMALL_SLABSUM = 448, SMALL_BYTES = 512;
// c->d_status: sub-arrays of tiles_cap u64 words each, in this order.  SA_STATUS's word
// ntiles - 1 is the slab aggregate k_finalize reads; the rest are SlabParams' pcnt, ppre,
// scan_look[0..1], tile_agg and tile_excl.
enum StatusArray : int { SA_STATUS, SA_PCNT, SA_PPRE, SA_LOOK0, SA_LOOK1, SA_TILE_AGG, SA_TILE_EXCL, STATUS_ARRAYS };

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Host copies between the caller's memory and the pinned staging buffers, split over a
// small persistent thread pool (one memcpy thread tops out near 25 GB/s, below PCIe Gen5).
class CopyPool {
 public:
  explicit CopyPool(int n);
  ~CopyPool();
  void copy(void *dst, const void *src, size_t n);
  // f(a, b) over disjoint 4 KiB-aligned slices of [0, n), one per thread (small n: inline)
  void parallel(size_t n, const std::function<void(size_t, size_t)> &f);

 private:
  void run(int i);
  const int nt_;
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(size_t, size_t)> *fn_ = nullptr;
  size_t n_ = 0;
  int pending_ = 0;
  unsigned long long gen_ = 0;
  bool stop_ = false;
};

}  // namespace sidx_host

// Device memory; node = a node body the tile passes stream (the context's input staging,
// shockidx_dev_alloc_node): physically contiguous when the driver can (hipDeviceMallocContiguous),
// else plain hipMalloc.  10 GiB FASTQ, interleaved allocations in one process on MI355X:
// k_fq_tiles 1.93-1.95 ms (median) from contiguous memory in 5 of 5 allocations, 1.92-2.15 ms from
// hipMalloc'd memory depending on where it landed (tools/placement_probe2.py,
// profiles/r04/placement2b.txt).  Written buffers (row tables, tile words) stay plain: the row
// placement ran 0.13 -> 0.18 ms into contiguous memory.  Freed with hipFree.
namespace sidx_host {
hipError_t dev_malloc(void **p, size_t bytes, bool node);
const DevAlloc *hip_allocator();  // dev_malloc / hipFree / hipGetErrorString
}  // namespace sidx_host

// The context.  Its device caches are the DevBuf members: each registers with `bufs`, which is
// what shockidx_ctx_workspace_bytes counts, what a trim drops (large buffers first, the tile block
// last) and what shockidx_ctx_destroy frees -- a new cache is one declaration here.  They grow on
// demand (DevBuf::ensure) and stay until a trim; the two slab slots are exact-size.  d_small,
// d_timing and the pinned host buffers are fixed-size, outside the count and the trims.
struct shockidx_ctx {
  typedef sidx::u64 u64;
  typedef sidx::u32 u32;
  template <class T, size_t PER = 1> using Buf = sidx_host::DevBuf<T, PER>;
  typedef sidx_host::BufClass BufClass;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ek0 = nullptr, ek1 = nullptr;
  hipEvent_t stage_ev[sidx_host::NSTAGE] = {nullptr, nullptr};
  sidx_host::BufSet bufs{sidx_host::hip_allocator()};
  Buf<uint8_t> d_in{bufs, BufClass::Large, true};  // input staging (node memory)
  Buf<u64, 2> d_rows{bufs};                        // the row table (capacity in rows)
  // the tile block: grown together by ensure_tiles for tiles_cap() tiles
  // (d_status: STATUS_ARRAYS sub-arrays of tiles_cap() words, StatusArray; d_detail: 4 words per
  // tile; d_fix: the k_fixup queue, FixRec of 24 bytes each, tiles_cap() items)
  Buf<u64> d_status{bufs, BufClass::Tile, false, "hipMalloc(status)"};
  Buf<u64> d_detail{bufs, BufClass::Tile, false, "hipMalloc(detail)"};
  Buf<u64> d_fix{bufs, BufClass::Tile, false, "hipMalloc(fix)"};
  u64 tiles_cap() const { return d_fix.cap / 4; }
  uint8_t *d_small = nullptr;  // badkey[2] | counters[2][NCOUNTERS] | result | detect
  u32 epoch = 0;               // build epoch for the look-back words (1..EPOCH_MASK)
  bool slots_dirty = false;    // a build took an epoch and did not reach its finalize
  int spec_fmt = 0;            // the last detected format (speculated by the next AUTO build)
  u64 *d_timing = nullptr;     // diagnostic phase timing buffer (SHOCKIDX_TIMING)
  u32 tiles_grid = 0;               // persistent grid of the tile passes (CUs x co-resident)
  u32 grid_cap = 0;                 // test hook (shockidx_debug_set_tiles_grid): the largest grid of any tile pass, 0: none
  uint8_t *h_stage[sidx_host::NSTAGE] = {nullptr, nullptr};
  sidx::DevResult *h_res = nullptr;
  sidx_host::CopyPool *pool = nullptr;  // host memcpy threads for the host-memory entry points
  Buf<uint8_t> d_sub{bufs};        // subset / gather workspace (bytes)
  int *h_det = nullptr;
  u64 ws_cap = 0;                  // SHOCKIDX_WORKSPACE_CAP: trim the caches above this after a call
  u64 dev_cap = 0;                 // device bytes a build may hold (0: what the device has free;
                                   //   shockidx_ctx_set_dev_cap / SHOCKIDX_DEV_CAP)
  Buf<u32> d_tile_stage{bufs};     // tile passes: staged positions (tile_stage_words() u32 entries)
  Buf<u32> d_tile_words{bufs};     //   per-tile results (FQ_TILE_WORDS per tile)
  Buf<uint8_t> d_cra{bufs};        // speculative chunkrecord: FASTQ record table / FASTA tile counts (bytes)
  Buf<uint8_t> d_crb{bufs};        //   node positions, jump tables, path, results (bytes)
  Buf<uint8_t> d_crc{bufs};        //   the slab walk's carry (bytes)
  // fd builds within the device cap: the two slab slots (exact-size, bytes each)
  Buf<uint8_t> d_slot[2] = {Buf<uint8_t>{bufs, BufClass::Large, true, "hipMalloc(slab slot)"},
                            Buf<uint8_t>{bufs, BufClass::Large, true, "hipMalloc(slab slot)"}};
  u32 cr_grid = 0;                 //   k_cr_verify persistent grid
  Buf<uint8_t> d_cola{bufs};       // column index: the line table, then the cut offsets (bytes)
  Buf<uint8_t> d_colb{bufs};       //   flags, ranks, key spans, scan workspace (bytes)
  Buf<uint8_t> d_plan{bufs};       // download plan: the level-2 workspace of CHUNK_RANGE (level 1 lives in d_sub)
  Buf<uint8_t> d_sec{bufs};        // sectioned stream: one large section staged 16-byte aligned, and its output (bytes)
  shockidx_stream_stats stream_stats = {};  //   how the last call's list was split (shockidx_stream_last_stats)
  Buf<uint8_t> d_batch{bufs};      // batch build: per-node formats, counts, first rows, slots, items, singles (bytes)
  Buf<uint8_t> d_bnodes{bufs};     //   the host entry point's node list (bytes)
  shockidx_batch_stats batch_stats = {};  //   how the last batch call ran (shockidx_batch_last_stats)
  Buf<uint8_t> d_sends{bufs};      // subset slab call: the window's line ends, their counts and scan workspace (bytes)
  Buf<uint8_t> d_spar{bufs};       // subset walk: the parent window (bytes)
  Buf<uint8_t> d_sruns{bufs};      //   the carry, then one slab's runs (bytes)
  shockidx_subset_stats subset_stats = {};  //   how the last file-level subset build ran (shockidx_subset_last_stats)
  Buf<uint8_t> d_fview{bufs};      // filter slab call: the window from the carried position on, 16-byte aligned (bytes)
  Buf<uint8_t> d_fout{bufs};       // filter walk / whole path: the carry, then one slab's (the section's) output (bytes)
  shockidx_filter_stats filter_stats = {};  //   how the last file-level filter call ran (shockidx_filter_last_stats)
  hipStream_t s_copy = nullptr;    // slab-pipelined host builds: the H2D stream
  uint8_t *h_rows[2] = {nullptr, nullptr};  // slab-pipelined fd builds: pinned row staging (D2H)
  // download filters over FASTQ: the tile pass keeps each record's line ends (k_fq_tiles<true>)
  bool want_spans = false;
  Buf<uint16_t> d_fqlines{bufs};   //   (u16 entries)
  sidx::SlabParams last_p;         // the last FASTQ tile pass's parameters (k_fq_spans_place)
  bool last_spans = false;         //   its line ends are in d_fqlines
  // test hooks (shockidx_debug_inject, not in the public header): bit0 a freshly grown status
  // array is filled with published words of the next build's epoch before it is zeroed, bit1
  // after it is zeroed (what a zeroing that lost a race with the build would leave), bit2 the
  // finalize reports one record short
  u32 inject = 0;
};

namespace sidx_host {

// ---- results and errors (the sink and set_msg: sidx_devbuf.hpp) ------------------------------
int set_hip(Err r, hipError_t e, const char *what);
template <class R> void reset_result(R *r) {
  if (r) memset(r, 0, sizeof *r);
}
// Go's text for a FASTQ status code (ST_*), nullptr for codes without one
const char *status_message(uint32_t code);

// (expects an error sink or a result pointer named res in scope)
#define HIPCHK(expr, what)                      \
  do {                                          \
    hipError_t _e = (expr);                     \
    if (_e != hipSuccess) return sidx_host::set_hip(res, _e, what); \
  } while (0)

// fasta.go:115-121: fmt.Errorf("Invalid fasta entry: %s", read[0:min(50, len(read))]) into res;
// read_piece(dst, k) fetches the piece's first k bytes (0, or its error code with res set).
template <class Read>
int fasta_error_text(Err res, uint64_t err_len, Read read_piece) {
  static const char pre[] = "Invalid fasta entry: ";
  char text[sizeof pre - 1 + 50];
  const uint64_t show = err_len < 50 ? err_len : 50;
  memcpy(text, pre, sizeof pre - 1);
  if (show)
    if (int rc = read_piece(text + sizeof pre - 1, show)) return rc;
  return set_msg(res, SHOCKIDX_EFORMAT, text, sizeof pre - 1 + show);
}

// carve 256-byte-aligned pieces out of a device workspace
struct Carver {
  uint8_t *base;
  sidx::u64 off = 0;
  template <class T> T *take(sidx::u64 n) {
    T *p = (T *)(base + off);
    off += (n * sizeof(T) + 255) / 256 * 256;
    return p;
  }
};

// one T from device memory, waited for
template <class T>
int d2h(shockidx_ctx *c, T *dst, const void *src, Err res) {
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(T), hipMemcpyDeviceToHost, c->stream), "subset copy");
  HIPCHK(hipStreamSynchronize(c->stream), "subset sync");
  return 0;
}
// the total of an exclusive scan of K > 0 lengths: off[K - 1] + len[K - 1], waited for
template <class L>
int scan_total(shockidx_ctx *c, const sidx::u64 *off, const L *len, sidx::u64 K, sidx::u64 *total, Err res) {
  sidx::u64 lo = 0;
  L ll = 0;
  if (int rc = d2h(c, &lo, off + K - 1, res)) return rc;
  if (int rc = d2h(c, &ll, len + K - 1, res)) return rc;
  *total = lo + ll;
  return 0;
}

// ---- the context's caches (sidx_build.cpp) -----------------------------------------------------
// device bytes held by the context's caches (c->bufs)
inline sidx::u64 workspace_bytes(const shockidx_ctx *c) { return c->bufs.bytes(); }
// free the large caches when the total is over `keep` (they regrow on demand); the tile block
// goes only with keep = 0, or when the rest is still over keep (BufSet::trim)
void trim_workspace(shockidx_ctx *c, sidx::u64 keep);
// the exact-size workspace of a slab walk (BufSet::exact): nothing happens when every size matches,
// else a trim to 0 and each buffer allocated in list order
int exact_workspace(shockidx_ctx *c, std::initializer_list<BufSet::Want> want, Err res);
// trims the caches to the context's cap when a host-facing call returns
struct TrimGuard {
  shockidx_ctx *c;
  ~TrimGuard() {
    if (c && c->ws_cap) trim_workspace(c, c->ws_cap);
  }
};
// Device bytes a build may hold: the context's cap, and never more than the device has free plus
// what this context already holds
sidx::u64 dev_budget(shockidx_ctx *c);
// what a one-pass build of an n-byte node holds at its peak
sidx::u64 one_pass_bytes(sidx::u64 n);

// ---- one index pass (sidx_build.cpp) ---------------------------------------------------------
// Slab geometry of one index pass (a single-GPU build is one slab = the whole file).
struct SlabGeom {
  sidx::u64 n, end, front, base, state_in, row_base;
  int eof, file_start;
  void *d_summary;
  sidx::u32 seq = 0;  // the summary's build tag (shockidx_slab.seq)
};
int resolve_format(shockidx_ctx *c, const uint8_t *d_data, sidx::u64 n, int kind, int fmt, hipStream_t s, int *kfmt,
                   Err res, const int **gate = nullptr);
int respeculate(shockidx_ctx *c, const sidx::DevResult &dr, int *kfmt, shockidx_result *res);
int run_index(shockidx_ctx *c, const uint8_t *d_data, sidx::u64 n, int kfmt, sidx::u64 *d_rows, sidx::u64 row_cap,
              hipStream_t s, sidx::DevResult *dr, shockidx_result *res, const SlabGeom *geom = nullptr,
              bool general = false, const int *gate = nullptr);
// one build's device work at a time per GPU: held around the kernels of a build (run_index takes it itself)
std::mutex &device_mutex(int device);
// SHOCKIDX_VERIFY is set (and not "0"): builds check their finished table on the device
bool verify_rows();
int translate(shockidx_ctx *c, const sidx::DevResult &dr, const uint8_t *d_data, hipStream_t s, shockidx_result *res);
int build_resident(shockidx_ctx *c, const uint8_t *d_data, sidx::u64 n, int kind, int fmt, hipStream_t s,
                   shockidx_result *res);

// ---- the download filters (sidx_filter_api.cpp) ------------------------------------------------
// filter.go:13-16: 1 fq2fa, 2 anonymize, 0 unknown
int filter_kind(const char *filter);
// one section (16-byte aligned, n bytes) through its filter; size_only: nothing written, out_cap
// ignored, the section's own status with the count / size a write would deliver
int filter_section(shockidx_ctx *c, int kind, const uint8_t *dd, sidx::u64 n, void *d_out, sidx::u64 out_cap,
                   shockidx_subset_result *res, bool size_only);

// ---- the download filters in slabs (sidx_filter_api.cpp, sidx_walks.cpp) -----------------------
// the device-side figures the walk's sizing takes (sidx_filtwalk.hpp) for views of len bytes
sidx::FiltWalkDev filter_walk_dev(shockidx_ctx *c, sidx::u64 len);
// One slab over the window [wlo, whi) of the section at win, bytes below own_end owned, the carry on
// the device.  Returns like shockidx_filter_slab_device (the format is FASTQ: detection is the
// caller's); waits for the stream.
int filter_slab_run(shockidx_ctx *c, int kind, const uint8_t *win, sidx::u64 wlo, sidx::u64 whi, sidx::u64 own_end,
                    bool first, bool last, sidx::u64 sec_size, sidx::FiltCarry *carry, uint8_t *d_out, sidx::u64 out_cap,
                    sidx::u64 *next_pos, shockidx_subset_result *res);
// shockidx_filter_fd: detection (anonymize), then the whole path or the walk
int filter_fd_any(shockidx_ctx *c, int kind, const char *filter, int fd, sidx::u64 off, sidx::u64 n, int out_fd,
                  shockidx_subset_result *res);
// The slab walk over the section [off, off + n) of fd (kind: filter_kind; S-byte slabs, 0: sized
// from the device budget; halo 0: the default), each slab's output to out_fd.  c->filter_stats says
// how it ran.
int filter_fd_walk(shockidx_ctx *c, int kind, const char *filter, int fd, sidx::u64 off, sidx::u64 n, int out_fd,
                   sidx::u64 S, sidx::u64 halo, shockidx_subset_result *res);

// ---- staging and copy-out (sidx_build.cpp) ---------------------------------------------------
// a row table the caller frees with free() / shockidx_free (2 MiB aligned when large)
uint64_t *alloc_rows_out(size_t bytes);
int rows_to_host(shockidx_ctx *c, const sidx::u64 *d_src, size_t bytes, uint8_t *dst, hipStream_t s,
                 Err res);
int fetch_rows(shockidx_ctx *c, sidx::u64 count, hipStream_t s, uint64_t **rows, shockidx_result *res);
// Host memory the GPU can DMA from directly (hipHostRegister'ed or hipHostMalloc'ed)
bool host_pinned(const void *p, sidx::u64 n);
// n bytes of pageable host memory / file bytes [off, off + n) into c->d_in (grown as needed)
int stage_host(shockidx_ctx *c, const void *data, sidx::u64 n, hipStream_t s, shockidx_result *res);
int stage_fd(shockidx_ctx *c, int fd, sidx::u64 off, sidx::u64 n, hipStream_t s, shockidx_result *res);
// Host bytes of a file for the pinned staging: pread until every byte of [off, off + k) has arrived
// (Linux returns at most 0x7ffff000 bytes per call; short reads and EINTR are retried).
struct PreadFill {
  int fd;
  Err res;
  CopyPool *pool;  // slices of each staging chunk are read by the pool's threads in parallel
  int operator()(uint8_t *dst, sidx::u64 off, size_t k) const;
};
// the process-wide budget of pinned page-cache bytes (pin_cap()): reserve before hipHostRegister,
// release after unregistering
bool pin_reserve(sidx::u64 b);
void pin_release(sidx::u64 b);

// ---- the slab pipelines (sidx_pipeline.cpp) --------------------------------------------------
// Where the rows of a slab-pipelined fd build go, as each slab's rows arrive in pinned host
// memory (called from the pipeline's index thread, rows in file order): the caller's table
// (shockidx_build_fd) or the temp .idx file (shockidx_create, pwrite at 16 * first row).
struct RowSink {
  virtual ~RowSink() {}
  virtual int put(const uint8_t *src, sidx::u64 first, sidx::u64 nrows, Err res) = 0;
};
struct TableSink : RowSink {  // a malloc'ed table, grown as rows arrive (the caller frees it)
  uint8_t *out = nullptr;
  size_t cap = 0;
  explicit TableSink(sidx::u64 n);
  ~TableSink() override;
  int put(const uint8_t *src, sidx::u64 first, sidx::u64 nrows, Err res) override;
};
struct FileSink : RowSink {  // the .idx temp file: rows are {u64 off, u64 len} LE (record.go:74-75)
  int fd = -1;
  int put(const uint8_t *src, sidx::u64 first, sidx::u64 nrows, Err res) override;
};
// ---- the column index in slabs (sidx_column_api.cpp, sidx_walks.cpp) ---------------------------
// One slab of the column slab pass: n owned bytes at d (16-byte aligned), `end` readable from d,
// `front` before it, d[0] at file offset base.  ws: sidx_col_tile_bytes(tiles of n, at least 1)
// bytes.  Returns like shockidx_column_slab_device; waits for the stream.
struct ColSlabIn {
  const uint8_t *d;
  sidx::u64 n, end, front, base, file_size;
  bool first, last;
};
int column_slab_run(shockidx_ctx *c, const ColSlabIn &sl, sidx::u32 column, void *ws, sidx::ColCarry *carry,
                    sidx::u64 *d_rows, sidx::u64 row_cap, hipStream_t s, shockidx_result *res);
// what the whole-node column build of an n-byte node holds at its peak: the node, its tile
// workspace and its rows (DevBuf::ensure's growth included)
sidx::u64 column_whole_bytes(sidx::u64 n);
// The slab walk over the file's n bytes (S-byte slabs, 0: sized from the device budget; halo 0:
// the default), rows to the sink slab by slab.  result->path 5.
int column_fd_walk(shockidx_ctx *c, int fd, sidx::u64 n, sidx::u32 column, sidx::u64 S, sidx::u64 halo, RowSink &sink,
                   shockidx_result *res);

// ---- the chunkrecord index in slabs (sidx_chunk_api.cpp, sidx_walks.cpp) -----------------------
// One slab of chunkrecord over the view v (sidx_common.hpp) with the carry on the device; first:
// the carry is initialised with fmt (later slabs take the format from it).  Rows at file offsets
// into rows[0..row_cap).  Returns like shockidx_chunkrecord_slab_device; waits for the stream.
int chunk_slab_run(shockidx_ctx *c, const sidx::ChunkView &v, sidx::u64 chunk, bool first, int fmt,
                   sidx::ChunkCarry *carry, sidx::u64 *rows, sidx::u64 row_cap, hipStream_t s, shockidx_result *res);
// what the whole-node chunkrecord build of an n-byte node holds at its peak (the node, its FASTQ
// record table or FASTA tile arrays, the graph, the rows), next to one_pass_bytes
sidx::u64 chunk_one_pass_bytes(shockidx_ctx *c, sidx::u64 n, sidx::u64 chunk);
// the device-side figures the walk's sizing takes (sidx_chunkwalk.hpp) for views of len bytes
sidx::ChunkWalkDev chunk_walk_dev(shockidx_ctx *c, sidx::u64 len);
// The slab walk over the file's n bytes (S-byte slabs, 0: sized from the device budget), rows to
// the sink slab by slab.  result->path 6.
int chunk_fd_walk(shockidx_ctx *c, int fd, sidx::u64 n, int fmt, sidx::u64 chunk, sidx::u64 S, RowSink &sink,
                  shockidx_result *res);

// ---- the subset indexes in slabs (sidx_subset_api.cpp, sidx_walks.cpp) -------------------------
// device bytes one slab call over a window of `end` readable bytes takes from the context's caches
// (c->d_sends, c->d_sub): 8 bytes per text byte for the line ends, the per-line arrays, the scans
sidx::u64 subset_slab_ws_bytes(sidx::u64 end);
void subset_slab_ws_parts(sidx::u64 end, sidx::u64 *ends_bytes, sidx::u64 *line_bytes);  // (c->d_sends, c->d_sub)
// what the whole build (shockidx_subset_index over the uploaded files) holds at its peak
sidx::u64 subset_whole_bytes(sidx::u64 ids_size, sidx::u64 parent_bytes);
// Where a walk's rows and runs go as each call delivers them (tables or temp files): first = the
// number of the first row / run of the piece
struct SubsetSinks {
  RowSink *rows, *runs;
};
// The walk over the two files: S-byte id slabs, W-row parent windows (0: sized from the device
// budget).  result as shockidx_subset_index's; c->subset_stats says how it ran.
int subset_fd_walk(shockidx_ctx *c, int ids_fd, sidx::u64 ids_size, int parent_fd, sidx::u64 parent_bytes,
                   sidx::i64 ilength, bool want_runs, sidx::u64 S, sidx::u64 W, SubsetSinks sinks,
                   shockidx_subset_result *res);

// *done = false: not applicable, the caller runs the plain path
int build_host_pipelined(shockidx_ctx *c, const void *data, sidx::u64 n, int kind, int fmt, uint64_t **rows,
                         shockidx_result *res, bool *done);
int build_fd_pipelined(shockidx_ctx *c, int fd, sidx::u64 n, int kind, int fmt, RowSink &sink, shockidx_result *res,
                       bool *done, bool *fell_back);

}  // namespace sidx_host
