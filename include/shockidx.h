/* shockidx.h -- C ABI of libshockidx, the MI355X (gfx950) record indexer for Shock.
 *
 * Drop-in boundary: this library replaces the body of the two Shock indexers that scan a
 * node's file, behind Shock's own plug-in registry
 *     index.Indexers = map[string]indexerFunc{ "record": ..., "line": ... }
 *     (shock-server/node/file/index/index.go:21-28)
 *     type Indexer interface { Create(string) (int64, string, error); Close() error }
 *     (shock-server/node/file/index/index.go:30-33)
 * A cgo shim registers NewGPURecordIndexer / NewGPULineIndexer under the
 * same keys; controller/node/index/index.go:176 and node/index.go:108-120 pick them up
 * unchanged.  Plain pointers and sizes only; no HIP or torch types in the signatures.
 *
 * Entry points and the reference code each one replaces (paths relative to
 * /root/reference/shock-server/):
 *   shockidx_create        record.Create / lineRecord.Create: index/record.go:34-90,
 *                          index/line.go:33-85 (scan + 16 MiB block writes + temp/rename)
 *   shockidx_build_fd      the scan of Create over the caller's *os.File (node/index.go:109-120)
 *   shockidx_build_host    the same over a POSTed body already in host memory
 *   shockidx_build_device  the device-resident core (input in HBM, table left in HBM)
 *   shockidx_detect        multi.Reader.DetermineFormat: format/multi/multi.go:43-62
 *   shockidx_write_idx     the .idx output protocol: index/record.go:35-41,65-87
 *   shockidx_chunkrecord_device  chunkRecord.Create (non-subset node): index/chunkrecord.go:41-99
 *   shockidx_chunkrecord_fd      the same over the node's *os.File (chunkrecord.go:43-56 reads it)
 *   shockidx_chunkrecord_subset_device  chunkRecord.Create for subset nodes (chunkrecord.go:100-228)
 *                          with fastq.go:216-243 / fasta.go:143-173 SeekChunk
 *   shockidx_column_device / shockidx_column_fd  CreateColumnIndex: index/column.go:33-130
 *   shockidx_column_slab_device / shockidx_column_fd_walk  the same loop (column.go:53-108) slab by slab
 *   shockidx_column_create  CreateColumnIndex with its temp file and rename (column.go:34-40,127)
 *   shockidx_subset_slab_device / shockidx_subset_fd_walk / shockidx_subset_create  the subset builders
 *       (index/subset.go:36-303) slab by slab and with their file protocol
 *   shockidx_download_plan the section list of a ?download&index=X&part=a&part=b... request, the
 *                          s.R = append(...) loops of controller/node/single.go:372-483 (Idx.Part /
 *                          Idx.Range per part, the subset node's chunkrecord branch :401-425) and
 *                          the virtual size index, index/virtual.go:50-80
 *
 * Semantics: results are bit-identical to the Go path on the same bytes, including the
 * exact error strings (fastq.go:156-207, fasta.go:120, errors.go:20) and the record count
 * reached before an error (the `count` Create returns alongside err).
 */
#ifndef SHOCKIDX_H
#define SHOCKIDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5: shockidx_slab.seq, the summary's build tag and shockidx_slab_combine's expect_seq (a stale
 *    summary is refused); row-capacity errors of build_device / chunkrecord / subset are
 *    SHOCKIDX_ESPACE (4 returned SHOCKIDX_EINVAL); whole-file builds check their own table's
 *    end invariants (SHOCKIDX_EINTERNAL instead of a short table).
 *    Added since without a version change (purely additive): shockidx_column_device,
 *    shockidx_column_fd, shockidx_stream_filter_device, shockidx_download_plan,
 *    shockidx_stream_last_stats, shockidx_build_batch_device, shockidx_build_batch_host,
 *    shockidx_batch_error, shockidx_batch_last_stats, shockidx_column_carry_bytes,
 *    shockidx_column_slab_device, shockidx_column_fd_walk, shockidx_column_create (and the code
 *    SHOCKIDX_EMORE, which only shockidx_column_slab_device returns), shockidx_subset_carry_bytes,
 *    shockidx_subset_slab_device, shockidx_subset_fd_walk, shockidx_subset_create,
 *    shockidx_subset_last_stats, shockidx_filter_carry_bytes, shockidx_filter_slab_device,
 *    shockidx_filter_fd_walk, shockidx_filter_fd, shockidx_filter_last_stats */
#define SHOCKIDX_ABI_VERSION 5

/* index kinds = the registry keys served (index/index.go:21-28) */
enum shockidx_kind { SHOCKIDX_RECORD = 0, SHOCKIDX_LINE = 1 };

/* formats (format/multi/multi.go:17-27) */
enum shockidx_format {
  SHOCKIDX_FMT_AUTO = -1, /* detect like multi.DetermineFormat (order fasta, fastq, sam) */
  SHOCKIDX_FMT_NONE = 0,
  SHOCKIDX_FMT_FASTA = 1,
  SHOCKIDX_FMT_FASTQ = 2,
  SHOCKIDX_FMT_SAM = 3,
  SHOCKIDX_FMT_LINE = 4 /* the line indexer (no detection, format/line/line.go) */
};

/* return codes */
enum shockidx_status {
  SHOCKIDX_OK = 0,
  SHOCKIDX_EFORMAT = 1,    /* reader/format error: Go's error string in result.err */
  SHOCKIDX_EMORE = 2,      /* shockidx_column_slab_device: a line does not close inside the slab's window;
                              result.state_out is its file offset (the caller's next move, not a failure) */
  SHOCKIDX_EINVAL = -1,
  SHOCKIDX_EHIP = -2,      /* HIP runtime error (result.err holds hipGetErrorString) */
  SHOCKIDX_ENOMEM = -3,
  SHOCKIDX_EIO = -4,       /* read/write/rename failure (errno text in result.err) */
  SHOCKIDX_EINTERNAL = -5, /* invariant violated on device (never expected) */
  SHOCKIDX_ESPACE = -6     /* output / record capacity too small: result.size (bytes) or
                              result.count (records) holds what the call needs */
};

typedef struct shockidx_ctx shockidx_ctx; /* one per concurrent caller (goroutine) */

typedef struct shockidx_result {
  uint64_t count;      /* records produced: Create's `count` (records before an error) */
  int32_t format;      /* SHOCKIDX_FMT_* that was indexed */
  int32_t status;      /* SHOCKIDX_OK or SHOCKIDX_EFORMAT (negative codes: system errors) */
  uint64_t err_len;    /* bytes in err (the FASTA message embeds raw file bytes) */
  char err[256];       /* Go error text, NUL-terminated */
  double kernel_ms;    /* device time of the index kernels (HIP events) */
  double h2d_ms;       /* host -> device staging time (host/fd entry points) */
  double d2h_ms;       /* table device -> host time */
  double total_ms;     /* wall time of the call */
  uint32_t path;       /* the build that ran last: 1 tile pass (one read of the input), 2 two-pass,
                          3 slab-pipelined build (build_host of a pinned FASTQ body, build_fd / create),
                          4 the same through two slab slots within the context's device cap
                          (shockidx_ctx_set_dev_cap), 5 the column index in slabs
                          (shockidx_column_slab_device, shockidx_column_fd_walk; a batch item: the batched walk),
                          6 chunkrecord in slabs (shockidx_chunkrecord_slab_device, shockidx_chunkrecord_fd_walk,
                          shockidx_chunkrecord_fd over the device cap); chunkrecord's whole-node build leaves 0 */
  uint32_t reruns;     /* builds re-run: a row-capacity overflow, a failed format speculation */
  double index_ms;     /* device time of the main index kernel alone (last pass) */
  uint64_t state_out;  /* format monoid state after the input (slab composition) */
  uint32_t term_code;  /* device status of the terminating record (diagnostic) */
  uint32_t flags;      /* device flags (diagnostic) */
  uint32_t fixups;     /* records / tiles re-validated from global memory (diagnostic) */
  uint32_t fix_tiles;  /* of which whole tiles re-indexed (diagnostic) */
} shockidx_result;

/* Context: owns a HIP stream on `device` plus cached device / pinned workspaces.
 * Thread-compatible: use one context per thread (or serialise calls on a context). */
int shockidx_ctx_create(int device, shockidx_ctx **out);
void shockidx_ctx_destroy(shockidx_ctx *ctx);
/* A context keeps its device workspaces (input staging, row table, tile status, scan and
 * subset space) grown to the largest call so far.  shockidx_ctx_trim frees them down to at
 * most keep_bytes (0: all; they regrow on demand); shockidx_ctx_workspace_bytes reports the
 * bytes held.  With SHOCKIDX_WORKSPACE_CAP=<bytes> in the environment at ctx_create, the
 * host-facing calls (build_host, build_fd, create, chunkrecord_fd) trim to the cap as they
 * return.  Not thread-safe against a concurrent call on the same context. */
int shockidx_ctx_trim(shockidx_ctx *ctx, uint64_t keep_bytes);
/* Device bytes one fd build (shockidx_build_fd / shockidx_create: the drop-in's Create) may hold;
 * 0 (default, or SHOCKIDX_DEV_CAP="2G" at context creation): what the device has free.  A node
 * whose one-pass build would not fit is indexed through two slab slots sized to the cap, so the
 * footprint does not grow with the node (record.go streams through a 4 KiB bufio.Reader,
 * record.go:51-83).  Replaces nothing in the reference (Go has no device memory); the shim
 * sets it from its pool configuration. */
int shockidx_ctx_set_dev_cap(shockidx_ctx *ctx, uint64_t bytes);
uint64_t shockidx_ctx_workspace_bytes(shockidx_ctx *ctx);

/* Device-resident build.  d_data: n bytes in HBM (16-byte aligned); d_rows: row_cap rows of
 * 16 bytes ({u64 offset, u64 length} LE).  stream: hipStream_t or NULL for the context's.
 * On return result->count rows are valid; if count > row_cap returns SHOCKIDX_ESPACE with
 * result->count = rows required (nothing beyond row_cap was written). */
int shockidx_build_device(shockidx_ctx *ctx, const void *d_data, uint64_t n, int kind, int fmt,
                          void *d_rows, uint64_t row_cap, void *stream,
                          shockidx_result *result);

/* Host-memory build (POSTed body).  *rows receives a malloc'ed table of result->count rows
 * (free with shockidx_free); on SHOCKIDX_EFORMAT it holds the rows before the error. */
int shockidx_build_host(shockidx_ctx *ctx, const void *data, uint64_t n, int kind, int fmt,
                        uint64_t **rows, shockidx_result *result);

/* Pin (hipHostRegister) / unpin a caller buffer, e.g. a node body kept in host memory for
 * several builds.  build_host detects pinned input (registered or hipHostMalloc'ed) and DMAs it
 * to HBM directly instead of copying it through the context's pinned staging. */
int shockidx_host_register(shockidx_ctx *ctx, void *p, uint64_t n);
int shockidx_host_unregister(shockidx_ctx *ctx, void *p);

/* File build over an open descriptor (not closed; read with pread from offset 0). */
int shockidx_build_fd(shockidx_ctx *ctx, int fd, uint64_t n, int kind, int fmt, uint64_t **rows,
                      shockidx_result *result);

/* Indexer.Create(outPath): build from fd then write <tmpdir>/<rand><rand>.idx and rename it
 * to outpath (record.go:35,87).  On a format error nothing is renamed into outpath. */
int shockidx_create(shockidx_ctx *ctx, int fd, uint64_t n, int kind, const char *tmpdir,
                    const char *outpath, shockidx_result *result);

/* Write `count` rows as an .idx file through a temp file + rename. */
int shockidx_write_idx(const uint64_t *rows, uint64_t count, const char *tmpdir,
                       const char *outpath, char *err, size_t errlen);

/* multi.DetermineFormat on the first min(n, 32768) bytes, run on the device.
 * *fmt = SHOCKIDX_FMT_FASTA/FASTQ/SAM or NONE; *mask = bit (f-1) set for every matching
 * validator (the reference ranges over a Go map, so overlapping matches are ambiguous). */
int shockidx_detect(shockidx_ctx *ctx, const void *data, uint64_t n, int *fmt, int *mask);

/* Device memory helpers on the context's device (for callers without their own HIP
 * allocator, e.g. a Go server holding a node resident in HBM).  Copies are synchronous. */
int shockidx_dev_alloc(shockidx_ctx *ctx, uint64_t bytes, void **d_ptr);
/* Device memory for a node body kept resident in HBM (what shockidx_build_device streams):
 * physically contiguous when the driver can provide it (the tile passes read it ~10 % faster
 * than memory hipMalloc places badly), else the same as shockidx_dev_alloc.  Free with
 * shockidx_dev_free. */
int shockidx_dev_alloc_node(shockidx_ctx *ctx, uint64_t bytes, void **d_ptr);
int shockidx_dev_free(shockidx_ctx *ctx, void *d_ptr);
int shockidx_memcpy_h2d(shockidx_ctx *ctx, void *d_dst, const void *src, uint64_t bytes);
int shockidx_memcpy_d2h(shockidx_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);
int shockidx_memset(shockidx_ctx *ctx, void *d_dst, int value, uint64_t bytes);
int shockidx_sync(shockidx_ctx *ctx); /* hipDeviceSynchronize on the context's device */
void *shockidx_stream(shockidx_ctx *ctx); /* the context's hipStream_t */

/* ---- Multi-GPU slabs ------------------------------------------------
 * A file too large for one GPU (or split for speed) is cut into byte slabs, one per GPU.
 * Each GPU indexes its slab against a *guessed* incoming reader state (the FASTQ line
 * phase, the FASTA '\n'-since-'>' bit, the SAM open-line class), the GPUs all-gather one
 * 64-byte summary each over RCCL, and a tiny device kernel folds the summaries in slab
 * order: it yields every slab's true incoming state (a wrong guess is re-run; it never is
 * on real data), the global number of the slab's first record and the global result. */
typedef struct shockidx_slab {
  const void *d_data; /* device pointer to the slab's first byte (16-byte aligned unless n == 0) */
  uint64_t n;         /* bytes owned by the slab (records starting here belong to it) */
  uint64_t end;       /* readable bytes from d_data: n + halo (records crossing the slab end) */
  uint64_t front;     /* readable bytes before d_data (>= 16; guesses look back up to 64 KiB) */
  uint64_t base;      /* file offset of d_data[0] */
  int32_t is_first;   /* slab starts at file offset 0 */
  int32_t is_last;    /* end is the end of the file */
  uint32_t seq;       /* the caller's build tag, stamped into the slab's summary */
  uint32_t reserved;
} shockidx_slab;

typedef struct shockidx_slab_summary { /* exchanged between GPUs; 64 bytes */
  uint64_t agg;      /* monoid aggregate of the slab bytes */
  uint64_t state_in; /* state the slab was indexed with */
  uint64_t key;      /* first-bad key (local record number << 28 | tile << 4 | status) or ~0 */
  uint64_t natural;  /* local record count if nothing terminated inside the slab */
  uint64_t row_base; /* local record number of the slab's first row */
  uint64_t err_pos;  /* FASTA error piece (file offset, length) */
  uint64_t err_len;
  uint16_t fmt;
  uint16_t flags;
  uint32_t seq;      /* shockidx_slab.seq of the build that wrote it */
} shockidx_slab_summary;

typedef struct shockidx_slab_plan { /* folded by every rank from all summaries */
  uint64_t state_in;     /* this slab's true incoming state */
  uint64_t first_record; /* global record number of this slab's rows[0] */
  uint64_t count;        /* global record count (Create's `count`) */
  uint64_t err_pos, err_len;
  uint32_t code;         /* device status of the terminating record */
  int32_t err_rank;      /* slab holding the error bytes (-1: none) */
  uint32_t inconsistent; /* bitmask of slabs whose guess was wrong (re-run them) */
  uint32_t flags;        /* 2: a device invariant failed, 4: a record ran past a halo,
                            32: a summary's seq was not the expected one (stale) */
} shockidx_slab_plan;

/* Guess the incoming state of a slab from its first bytes and the bytes before it. */
int shockidx_slab_guess(shockidx_ctx *ctx, const shockidx_slab *slab, int fmt, uint64_t *state_guess);
/* Index one slab with `state_in`; rows of the slab's records go to d_rows[0..), the 64-byte
 * summary to d_summary (device memory).  Asynchronous on the context stream. */
int shockidx_slab_index(shockidx_ctx *ctx, const shockidx_slab *slab, int fmt, uint64_t state_in,
                        void *d_rows, uint64_t row_cap, void *d_summary, shockidx_result *result);
/* Fold `world` gathered summaries (device memory, slab order) into this rank's plan.
 * expect_seq (host memory, `world` tags, or NULL: unchecked): the seq each slab's summary must
 * carry -- the tag its latest shockidx_slab_index was given; any other sets plan->flags 32. */
int shockidx_slab_combine(shockidx_ctx *ctx, const void *d_all, int world, int rank, int fmt,
                          const uint32_t *expect_seq, shockidx_slab_plan *plan);

/* RCCL communicator (one per process / GPU).  The 128-byte unique id is created by rank 0
 * and broadcast by the caller (e.g. over a CPU process group). */
typedef struct shockidx_comm shockidx_comm;
int shockidx_comm_unique_id(void *id128);
int shockidx_comm_init(shockidx_ctx *ctx, int world, int rank, const void *id128, shockidx_comm **out);
int shockidx_comm_allgather(shockidx_comm *comm, const void *d_send, void *d_recv, uint64_t bytes);
int shockidx_comm_destroy(shockidx_comm *comm);
/* ranks the communicator spans (ncclCommCount): what a run reports as the ranks its
 * all-gather actually crossed over RCCL (bench.py --gpus N: "rccl_ranks") */
int shockidx_comm_count(const shockidx_comm *comm, int *nranks);

/* ---- One file across several GPUs from one process -------------------
 * The Shock server is one process: node.AsyncIndexer builds an index in a goroutine
 * (node/index.go:107-121) and never sees ranks.  A multi-device group cuts the node file into
 * byte slabs, one per device, stages each slab (plus 64 KiB before and a 4 MiB halo after it)
 * into its GPU, indexes them concurrently with the tile passes against guessed incoming
 * states, all-gathers the 64-byte slab summaries over RCCL (one communicator per device,
 * ncclCommInitAll; 64 B x n is all that crosses xGMI), folds them on every device, re-runs a
 * slab whose guess was wrong and concatenates the owned rows: the table, count and Go error
 * text equal shockidx_build_host's.  devices[k] takes slab k; a device may be listed more than
 * once (its slabs then run one after another and the summaries go through host memory).  A
 * record longer than the halo crossing a slab end is built on devices[0] alone. */
typedef struct shockidx_multi shockidx_multi;
/* visible GPUs (hipGetDeviceCount); 0 when there is no usable GPU */
int shockidx_device_count(void);
int shockidx_multi_create(const int *devices, int n_devices, shockidx_multi **out);
void shockidx_multi_destroy(shockidx_multi *m);
/* 1: the summaries are all-gathered over RCCL; 0: through host memory */
int shockidx_multi_rccl(const shockidx_multi *m);
/* shockidx_build_host / shockidx_build_fd / shockidx_create across the group's devices */
int shockidx_multi_build_host(shockidx_multi *m, const void *data, uint64_t n, int kind, int fmt, uint64_t **rows,
                              shockidx_result *result);
int shockidx_multi_build_fd(shockidx_multi *m, int fd, uint64_t n, int kind, int fmt, uint64_t **rows,
                            shockidx_result *result);
int shockidx_multi_create_index(shockidx_multi *m, int fd, uint64_t n, int kind, const char *tmpdir,
                                const char *outpath, shockidx_result *result);
/* Device-resident form (benchmarks; a server keeping node bodies in HBM).  Slab k of a file of
 * `size` bytes owns [lo[k], hi[k]) and is held as window [wlo[k], whi[k]) at d_win[k] on
 * devices[k] (shockidx_multi_plan).  Rows stay on the devices: d_rows[k] (row_cap[k] rows)
 * receives the slab's rows, the first rows_owned[k] of which are global records
 * first_record[k]..  Returns like shockidx_build_device (result->count = global count); a row_cap[k]
 * too small for its slab returns SHOCKIDX_ESPACE with result->count = the most rows any short
 * slab needs. */
int shockidx_multi_plan(const shockidx_multi *m, uint64_t size, uint64_t *lo, uint64_t *hi, uint64_t *wlo,
                        uint64_t *whi);
int shockidx_multi_build_resident(shockidx_multi *m, uint64_t size, int kind, int fmt, const void *const *d_win,
                                  void *const *d_rows, const uint64_t *row_cap, uint64_t *first_record,
                                  uint64_t *rows_owned, shockidx_result *result);

/* ---- Subset nodes (BASELINE config C4) -------------------------
 * A subset node is built from an uploaded list of 1-based record ids (one per line) over the
 * parent's record index: index/subset.go:133-303 CreateSubsetNodeIndexes writes one parent
 * row per id (<node>/idx/<parent index>.idx) and the maximal runs of contiguous rows
 * (<node>/<id>.subset.idx); reading the subset node streams those runs of the parent file
 * (controller/node/single.go:500-517, request/streamer.go:58-117). */
typedef struct shockidx_subset_result {
  uint64_t count;    /* oCount: subset index rows (rows written before an error) */
  uint64_t runs;     /* coCount: compressed index rows */
  uint64_t size;     /* oSize: bytes of the subset node (sum of the row lengths) */
  int32_t status;    /* SHOCKIDX_OK, SHOCKIDX_EFORMAT (Go's error text in err) or < 0 */
  uint32_t pad;
  uint64_t err_len;
  char err[256];
  double kernel_ms;  /* device time: the subset kernels (index) / k_gather (gather) */
  double total_ms;
  double gather_ms;  /* shockidx_subset_node: device time of k_gather */
} shockidx_subset_result;

/* CreateSubsetNodeIndexes on device memory.  d_ids: the id text (ids_len bytes, 16-byte
 * aligned); d_parent: parent_count parent rows {u64 off, u64 len}; ilength: the parent
 * index's TotalUnits.  Writes result->count rows to d_rows and result->runs rows to d_runs
 * (capacities in rows; a short capacity returns SHOCKIDX_ESPACE with the needed counts). */
int shockidx_subset_index(shockidx_ctx *ctx, const void *d_ids, uint64_t ids_len, const void *d_parent,
                          uint64_t parent_count, int64_t ilength, void *d_rows, uint64_t rows_cap, void *d_runs,
                          uint64_t runs_cap, shockidx_subset_result *result);

/* The subset node's bytes: the runs of the parent file d_data (data_len bytes) concatenated
 * into d_out (out_cap bytes; result->size = bytes written, or needed with SHOCKIDX_ESPACE). */
int shockidx_subset_gather(shockidx_ctx *ctx, const void *d_data, uint64_t data_len, const void *d_runs,
                           uint64_t nruns, void *d_out, uint64_t out_cap, shockidx_subset_result *result);

/* shockidx_subset_index and shockidx_subset_gather in one call: the counts between them stay
 * on the device, so the host waits only for the id line count and the result.  d_runs is
 * required; d_out receives the node's bytes when the index succeeds (result->size bytes). */
int shockidx_subset_node(shockidx_ctx *ctx, const void *d_ids, uint64_t ids_len, const void *d_parent,
                         uint64_t parent_count, int64_t ilength, void *d_rows, uint64_t rows_cap, void *d_runs,
                         uint64_t runs_cap, const void *d_data, uint64_t data_len, void *d_out, uint64_t out_cap,
                         shockidx_subset_result *result);

/* CreateSubsetIndex (index/subset.go:36-128; caller node/index.go:103): the subset index of
 * a node from an id list over a parent index -- the per-id checks and rows of
 * shockidx_subset_index without the compressed index.  On a Go error (SHOCKIDX_EFORMAT)
 * result->count = result->size = UINT64_MAX, i.e. Go's (-1, -1, err) read as int64. */
int shockidx_create_subset_index(shockidx_ctx *ctx, const void *d_ids, uint64_t ids_len, const void *d_parent,
                                 uint64_t parent_count, int64_t ilength, void *d_rows, uint64_t rows_cap,
                                 shockidx_subset_result *result);

/* ---- subset indexes in slabs and from files ---------------------------------------------------
 * The same two builders (index/subset.go:133-303 and :36-128) walking the id text slab by slab and
 * the parent index window by window, so that the device holds two id slots, a parent window, one
 * slab's workspace and one slab's rows and runs however long the id list is.  subset.go's loop
 * carries prev_int, prevOffset, prevLength, coOffset, coLength and the three counters from line to
 * line (:161-176); a slab call takes them from the carry and leaves them in it.
 *
 * The id slab (shockidx_slab): d_data 16-byte aligned; n owned bytes, end readable bytes from d_data
 * (n + halo), front readable bytes before it (at least 16 unless base < 16, then base); base, the
 * offset of d_data[0] in the id text, may be any offset and n any length; is_first: base == 0;
 * is_last: base + n == ids_size; seq is ignored.  A line starts at offset 0 or after a '\n'.  The
 * call owns the lines that start in [max(base, carry.next_off), base + n), carry.next_off being the
 * first line not yet consumed.  d_carry: shockidx_subset_carry_bytes() bytes of device memory,
 * 8-byte aligned, zeroed before a walk's first slab, which initialises it (a header and two halves
 * of the state: a call reads one half and writes the other); the host never reads it.  No byte
 * outside [d_data - front, d_data + end) is read.
 *
 * The parent window: d_parent (16-byte aligned) holds rows [prow0, prow0 + prows) of the parent
 * index, parent_count is the number of whole rows in the parent file; no row outside the window is
 * read, the previous id's row comes from the carry.
 *
 * A call consumes its owned lines in order exactly as subset.go:186-272 does: a line of at most one
 * byte is skipped (:197-199), strconv.Atoi of buf[:n-1] (:201-206), the sort check against the
 * previous accepted id (the carry's for the call's first line, :208-211), the check against ilength
 * (:213-216), the failed ReadAt, an id above parent_count (:218-223).  Each accepted id's row goes
 * to d_rows; with want_runs every run closed by a consumed id goes to d_runs as (coOffset, coLength)
 * (:245-261), the open run stays in the carry, and the last slab, once every line is consumed,
 * writes the final run iff oSize != 0 (:285-291; rows all of length 0 leave none).  The bytes after
 * the last '\n' are dropped (:187-195).
 *
 * result->stop and result->next_off say where the call stopped; every line before next_off is
 * consumed and the carry has advanced: 0 all owned lines consumed; 1 the line at next_off does not
 * close inside the window, which does not reach ids_size; 2 the id at next_off (result->next_id)
 * passed every check but its row next_id - 1 lies outside the window -- the same slab submitted
 * again with another window goes on from there.  Of an error line and a stop line the earlier one
 * decides.
 *
 * Returns SHOCKIDX_OK: result->rows / runs written by this call, and the running totals count,
 * nruns, size (oCount, coCount, oSize).  SHOCKIDX_EFORMAT: Go's text, as shockidx_subset_index
 * gives it for the whole input; the rows and closed runs before the failing id are written, the
 * totals are Go's at that point (the open run is not counted), and the walk has ended: any later
 * call is SHOCKIDX_EINVAL, as is one after the last slab has finished.  SHOCKIDX_ESPACE:
 * result->rows / runs hold what the call needs, the carry is unchanged, and the same call with
 * larger tables succeeds.  SHOCKIDX_EINVAL: carry.next_off lies before the slab's first byte (the
 * line there would belong to no slab) or at or past its last (the walk is past this slab, or the
 * carry is left from an abandoned walk and was not zeroed), the walk is over, or an argument is
 * misaligned.  The calls' rows concatenated are shockidx_subset_index's
 * d_rows, their runs its d_runs, the final totals its totals. */
typedef struct shockidx_subset_slab_result {
  uint64_t rows;      /* rows written to d_rows by this call (SHOCKIDX_ESPACE: needed) */
  uint64_t runs;      /* runs written to d_runs by this call (SHOCKIDX_ESPACE: needed) */
  uint64_t count;     /* oCount so far */
  uint64_t nruns;     /* coCount so far */
  uint64_t size;      /* oSize so far */
  uint64_t next_off;  /* the line the call stopped at */
  int64_t next_id;    /* stop 2: the id whose row the window lacks */
  int32_t stop;       /* 0, 1 or 2 */
  int32_t status;
  uint64_t err_len;
  char err[256];
  double kernel_ms;
  double total_ms;
} shockidx_subset_slab_result;
uint64_t shockidx_subset_carry_bytes(void);
int shockidx_subset_slab_device(shockidx_ctx *ctx, const shockidx_slab *ids_slab, uint64_t ids_size,
                                const void *d_parent, uint64_t prow0, uint64_t prows, uint64_t parent_count,
                                int64_t ilength, int want_runs, void *d_carry, void *d_rows, uint64_t rows_cap,
                                void *d_runs, uint64_t runs_cap, shockidx_subset_slab_result *result);

/* The walk over two open descriptors (not closed; pread): id slabs in file order, slab k + 1
 * crossing PCIe into the second slot while slab k runs (halo 64 KiB); the first parent window
 * starts at row 0 and after stop 2 the next one starts at row next_id - 1, so sparse lists skip
 * rows and dense ones abut; parent_count = parent_bytes / 16.  Each call's rows and runs go to the
 * host as they are made: *rows / *runs receive malloc'ed tables of result->count / result->runs
 * rows (free with shockidx_free; runs may be NULL without want_runs).  ids_slab_bytes /
 * parent_slab_rows 0: sized so that the two id slots, the parent window, one slab's workspace (8
 * bytes per text byte included) and its rows and runs fit the context's device budget
 * (shockidx_ctx_set_dev_cap); a budget under 32 MiB is SHOCKIDX_ENOMEM, as is an id line longer
 * than a slab slot can hold.  On SHOCKIDX_EFORMAT the tables hold what was written before the
 * error and result is as shockidx_subset_index's. */
int shockidx_subset_fd_walk(shockidx_ctx *ctx, int ids_fd, uint64_t ids_size, int parent_fd, uint64_t parent_bytes,
                            int64_t ilength, int want_runs, uint64_t ids_slab_bytes, uint64_t parent_slab_rows,
                            uint64_t **rows, uint64_t **runs, shockidx_subset_result *result);
/* CreateSubsetNodeIndexes' file protocol (subset.go:136-158,274-297; callers node/fs.go:52-126),
 * and with cofile == NULL CreateSubsetIndex's (:36-128; node/index.go:103: no runs, and on a Go
 * error count = size = UINT64_MAX).  Within the budget today's whole build over the uploaded
 * files, else the walk, which writes each table at 16 * row as it goes.  The tables go through temp
 * files in tmpdir; cofile is renamed first, then ofile (:293-297).  On any error nothing is left at
 * either path or in tmpdir (the reference leaves its temp files behind). */
int shockidx_subset_create(shockidx_ctx *ctx, int ids_fd, uint64_t ids_size, int parent_fd, uint64_t parent_bytes,
                           int64_t ilength, const char *tmpdir, const char *cofile, const char *ofile,
                           shockidx_subset_result *result);
/* how the context's last shockidx_subset_fd_walk / shockidx_subset_create ran */
typedef struct shockidx_subset_stats {
  uint64_t walked;       /* 1: the slab walk, 0: the whole build */
  uint64_t calls;        /* slab calls */
  uint64_t slabs;        /* id slabs */
  uint64_t windows;      /* parent windows uploaded */
  uint64_t ids_bytes;    /* id text bytes sent to the device */
  uint64_t parent_bytes; /* parent index bytes sent to the device */
  uint64_t slab_bytes;   /* the id slab size used */
  uint64_t window_rows;  /* the parent window size used */
  uint64_t held_bytes;   /* device bytes the context's caches held when the build ended */
} shockidx_subset_stats;
int shockidx_subset_last_stats(const shockidx_ctx *ctx, shockidx_subset_stats *out);

/* ---- Index read path: Idx.Part / Idx.Range ----------------------
 * index/index.go:67-117 and :119-193 (callers: controller/node/single.go:391-508,
 * controller/preauth/preauth.go:84) over an index resident in HBM: d_rows holds the .idx
 * file's nrows rows {u64 offset, u64 length}; d_rows == NULL stands for a missing file
 * (IndexNoFile).  part: the request's part value ("N" or "N-M", strconv.ParseInt semantics,
 * strings.Split on '-'); idx_length: the index's TotalUnits.  Go's error text
 * (IndexNoFile / InvalidIndexRange / IndexOutBounds) comes back with SHOCKIDX_EFORMAT.
 * A row past the table reads like Go's failed binary.Read: Part sees zeros; Range keeps the
 * last row it read.  Part: *pos, *length = Go's (pos, length), int64 arithmetic. */
int shockidx_idx_part(shockidx_ctx *ctx, const void *d_rows, uint64_t nrows, const char *part, int64_t idx_length,
                      int64_t *pos, int64_t *length, shockidx_subset_result *result);
/* Range: result->count {int64 pos, int64 length} records (maximal runs of contiguous rows) in
 * d_recs (recs_cap records; a short capacity returns SHOCKIDX_ESPACE with the needed count).
 * end < start gives an empty list, like Go's loop. */
int shockidx_idx_range(shockidx_ctx *ctx, const void *d_rows, uint64_t nrows, const char *part, int64_t idx_length,
                       void *d_recs, uint64_t recs_cap, shockidx_subset_result *result);

/* ---- Download filters --------------------------------------------
 * node/filter/filter.go:13-16 "fq2fa" (fq2fa/fq2fa.go:58-84) and "anonymize"
 * (anonymize/anonymize.go:28-56) over one FASTQ section (d_data, n bytes in HBM) into d_out:
 * the stream the filter's Read delivers -- every record fastq.Reader.Read (fastq.go:50-132)
 * returns without error, formatted (fq2fa: ">" ID "\n" Seq "\n"; anonymize: "@" counter
 * "\n" Seq "\n+\n" Qual "\n", counter from 1); a record returned together with io.EOF
 * (quality line without '\n' at the end) is dropped like the reference drops it.  Reader
 * errors end the stream: SHOCKIDX_EFORMAT with Go's text, result->count / size = records /
 * bytes delivered before it.  anonymize detects the format (multi.go:43-62): over a FASTA
 * section every sequence fasta.Reader.Read returns (fasta.go:40-88) as ">" counter "\n" Seq "\n"
 * (the sequence read with io.EOF dropped; "Invalid fasta entry" ends the stream), over a SAM
 * section every alignment line sam.Reader.Read returns (sam.go:44-81) as the trimmed line +
 * "\n" ("sam alignment fields less than 11").  A short out_cap returns SHOCKIDX_ESPACE with
 * result->size = the bytes needed. */
int shockidx_filter_device(shockidx_ctx *ctx, const char *filter, const void *d_data, uint64_t n, void *d_out,
                           uint64_t out_cap, shockidx_subset_result *result);

/* ---- The sectioned stream: request.Streamer.Stream with a Filter --------------------------
 * request/streamer.go:78-98 over sections of a node resident in HBM: the Streamer holds a list of
 * SectionReaders and builds a new filter reader for each (s.Filter(sr), :86-87); for a subset node
 * the list is every row Idx.Range returns (controller/node/single.go:397-400, 442-444, 457-460,
 * 505-516).  d_secs: nsecs records {int64 pos, int64 len}, the layout shockidx_idx_range writes, so
 * Range -> stream needs no host trip.  Sections may touch, overlap, repeat and come in any order.
 * The result is that of shockidx_filter_device on section 0, 1, 2, ... alone, each over exactly the
 * bytes [pos, pos + len), the outputs concatenated in list order: a section's end is end of file for
 * its reader (a record whose quality line has no '\n' before it is dropped, in every section), the
 * anonymize counter restarts at 1 and the format is detected again in every section
 * (anonymize.go:28-56, multi.go:43-62; an empty section is "Invalid file type for filter"), and
 * fq2fa over an empty section delivers nothing.  The stream stops after the first section whose
 * status is not SHOCKIDX_OK (io.Copy's error, streamer.go:91-96): its delivered bytes are kept,
 * nothing follows them, the call returns its status and text, and *err_section (optional) receives
 * its index -- Streamer.ESection (:92-95) -- or -1.  result->count / size: records / bytes
 * delivered over all sections.  A short out_cap returns SHOCKIDX_ESPACE with result->size = the
 * bytes needed and nothing written.  A section with pos < 0, len < 0 or pos + len > data_len is
 * SHOCKIDX_EINVAL and nothing is written: the reference's SectionReader would see a short read
 * there, and a valid index never produces such a row.  filter NULL or "" is the Streamer without a
 * Filter (:88-90): shockidx_subset_gather of the sections.  d_data and d_out 16-byte aligned.
 * Small sections -- at most SHOCKIDX_STREAM_SMALL bytes (environment, applies to every format; the
 * defaults are per format, DESIGN.md "The sectioned stream") and FASTQ, FASTA or SAM (as detected per
 * section under anonymize; fq2fa reads everything as FASTQ) -- are indexed together, every maximal run
 * of consecutive small sections of one format in a number of launches and host waits that does not
 * grow with the run's length; the others (too long, or of no detected format) go through the
 * single-section filter one at a time. */
int shockidx_stream_filter_device(shockidx_ctx *ctx, const char *filter, const void *d_data, uint64_t data_len,
                                  const void *d_secs, uint64_t nsecs, void *d_out, uint64_t out_cap,
                                  int64_t *err_section, shockidx_subset_result *result);

/* Which path the context's last shockidx_stream_filter_device call with a filter took (the stream
 * delivered does not depend on it). */
typedef struct shockidx_stream_stats {
  uint64_t sections;     /* nsecs of the context's last shockidx_stream_filter_device call with a filter */
  uint64_t batches;      /* groups that took the segmented path (counted once, not per walk) */
  uint64_t batched;      /* sections inside them */
  uint64_t singles;      /* sections that went through the single-section filter */
  uint64_t by_format[3]; /* batches of FASTQ, FASTA, SAM sections */
} shockidx_stream_stats;
int shockidx_stream_last_stats(const shockidx_ctx *ctx, shockidx_stream_stats *out);

/* ---- The download filters in slabs: a section of a node file through two device slots ------
 * GET /node/{id}?download&filter=F streams the whole file through one filter reader
 * (controller/node/single.go:490-526, Streamer{R: []SectionReader{nf}}), its seek / length form one
 * section of it (single.go:194-257).  These entry points do that for a FASTQ section of any size
 * with a bounded device footprint: fq2fa always, anonymize when the section detects as FASTQ.
 * Offsets are section offsets: section byte 0 is the reader's offset 0, the section's end its EOF.
 *
 * shockidx_filter_slab_device: one slab.  The window is the section bytes [base - front, base + end);
 * d_data is the 16-byte-aligned device address of section byte base; base may be any offset and
 * front may be 0 (no byte before the carried position is needed).  n <= end is the bytes owned: a
 * Read (fastq.go:50-132) that starts before base + n belongs to this slab, one that starts at or
 * after it to the next.  is_last != 0 exactly when base + end == sec_size (with n == end that slab
 * owns the Read at the section's very end too and ends the stream; with n < end it leaves the Reads
 * from base + n on to a further is_last slab); seq is ignored; no byte outside the window is read.
 * d_carry:
 * shockidx_filter_carry_bytes() bytes of device memory, 8-byte aligned, holding in two halves (a slab
 * reads one and writes the other) the position of the next Read, the records and bytes delivered,
 * the filter and an ended flag; is_first initialises it (position 0).
 *   A record is settled by a slab that is not the last when, from its Read's start, the blank lines
 * Read skips (fastq.go:57-68) and the four lines after them each find their '\n' before base + end;
 * on the last slab everything is settled with the section's end as EOF (the record returned with
 * io.EOF is dropped, the "truncated" errors fire, blank lines at EOF end the stream cleanly).  The
 * slab delivers, in order, every owned record up to the first that is not settled or that fails.
 *   SHOCKIDX_OK: result->count records and result->size bytes were written to d_out (both may be
 *     0), *next_pos is the carried position; after the last slab the carry is ended.
 *   SHOCKIDX_EFORMAT: Go's text; count / size and d_out hold what was delivered before it; the
 *     carry is ended.  anonymize over a first slab of no format: "Invalid file type for filter".
 *   SHOCKIDX_ESPACE: result->size is the bytes this slab needs; nothing is written.
 *   SHOCKIDX_EINVAL: the carry is ended or was made by the other filter, the carried position lies
 *     outside [base - front, base + n], the first slab of anonymize does not hold the section's
 *     first min(32768, sec_size) bytes from a 16-byte-aligned address (detection reads them), or it
 *     detects as FASTA or SAM (those sections are not walked; the text says so).
 * Anything but SHOCKIDX_OK or SHOCKIDX_EFORMAT leaves the carry as it was.  Concatenated over the
 * slabs of a walk, d_out is what shockidx_filter_device writes for the whole section, the final
 * status and text are the same, and the carried counts are the whole call's.
 *
 * shockidx_filter_fd_walk: the section [off, off + n) of fd, always slab by slab (slab_bytes 0:
 * sized from the device budget, which must be at least 32 MiB; halo_bytes 0: the column walk's
 * default, less under a small budget), slab k + 1 crossing PCIe while slab k runs, each slab's
 * output written to out_fd in order with write(2) -- out_fd may be a pipe (no lseek, no pwrite;
 * short writes and EINTR are handled; a failed write is SHOCKIDX_EIO with the errno text).  The bytes
 * delivered before a SHOCKIDX_EFORMAT are written before the call returns (io.Copy delivers them
 * before the reader's error, request/streamer.go:91-96).  A record that no slot can hold is
 * SHOCKIDX_ENOMEM after the earlier bytes were written, never a short stream returned as success.
 * result->count / size: records / bytes delivered.
 *
 * shockidx_filter_fd: the whole path (the section, its output and the workspace resident at once)
 * when that fits the device budget by a worst-case bound, else the walk.  anonymize detects from
 * the section's first 32 KiB first: FASTQ as above; FASTA and SAM take the whole path, or
 * SHOCKIDX_ENOMEM with a text naming the format when they do not fit; no format is SHOCKIDX_EFORMAT
 * with nothing written. */
uint64_t shockidx_filter_carry_bytes(void);
int shockidx_filter_slab_device(shockidx_ctx *ctx, const char *filter, const shockidx_slab *slab,
                                uint64_t sec_size, void *d_carry, void *d_out, uint64_t out_cap,
                                uint64_t *next_pos, shockidx_subset_result *result);
int shockidx_filter_fd_walk(shockidx_ctx *ctx, const char *filter, int fd, uint64_t off, uint64_t n, int out_fd,
                            uint64_t slab_bytes, uint64_t halo_bytes, shockidx_subset_result *result);
int shockidx_filter_fd(shockidx_ctx *ctx, const char *filter, int fd, uint64_t off, uint64_t n, int out_fd,
                       shockidx_subset_result *result);

/* How the context's last shockidx_filter_fd / shockidx_filter_fd_walk call ran. */
typedef struct shockidx_filter_stats {
  uint64_t path;        /* 1: the whole path, 2: the walk */
  uint64_t slabs;       /* slab calls that ran (the walk) */
  uint64_t restarts;    /* slabs restarted at a record its halo did not settle */
  uint64_t slab_bytes;  /* the walk's slab and halo */
  uint64_t halo_bytes;
  uint64_t peak_bytes;  /* device bytes the context's caches held at the call's end (its peak) */
  uint64_t kernel_us;   /* where the call's time went: device work, the output's way to the host, */
  uint64_t d2h_us;      /*   write(2), */
  uint64_t write_us;
} shockidx_filter_stats;
int shockidx_filter_last_stats(const shockidx_ctx *ctx, shockidx_filter_stats *out);

/* ---- The download plan: all parts of an index download in one call -------------------------
 * controller/node/single.go:372-483 builds the Streamer's section list (s.R) part by part: a request
 * may repeat part= any number of times, every part is one Idx.Part section or the records of one
 * Idx.Range, appended in order, and the request fails at the first part in error (nothing is
 * streamed).  This call does that for the whole list at once, over indexes resident in HBM, in a
 * number of launches and host waits that does not grow with nparts.  d_secs receives result->count
 * records {int64 pos, int64 len} -- what the reference appends to s.R, in its order, the layout
 * shockidx_idx_range writes and shockidx_stream_filter_device reads -- and result->size is Go's
 * `size` (single.go:369, the int64 sum of the lengths, wrapping).  Modes: */
enum shockidx_plan_mode {
  SHOCKIDX_PLAN_PART = 0,        /* idx.Part per part: single.go:461-475 (non-subset index of a file) */
  SHOCKIDX_PLAN_RANGE = 1,       /* idx.Range per part: single.go:433-460, 505-516 (subset index / subset node) */
  SHOCKIDX_PLAN_CHUNK_RANGE = 2, /* subset node + chunkrecord: single.go:401-425 (Range, then Range per chunk run) */
  SHOCKIDX_PLAN_SIZE = 3         /* the virtual size index: virtual.go:50-80 with single.go:357-366's chunk_size */
};
/* PART: one section per part with Idx.Part's arithmetic (index.go:86-114); a row past the table
 * reads as zeros.  RANGE: the sections of part 0, then part 1, ...; each part's are Idx.Range's
 * maximal runs (curLen == nextPos - curPos, index.go:152-177), "N" and "N-N" one record, b < a none;
 * a row past the table reads as the last row read in that part's walk (zeros when its first row is
 * past the table); sections of different parts never merge, also when they touch, overlap or
 * repeat.  CHUNK_RANGE: RANGE over d_rows, the "matrix" index of shockidx_chunkrecord_subset_device
 * (rows (16 * first row, 16 * rows)); every record (c0, c1) it yields, in order, becomes
 * start = c0/16 + 1, stop = (start-1) + c1/16 (int64, truncating, wrapping) and the sections are
 * Idx.Range("start-stop") over d_rec_rows with rec_length (single.go:411-423): start == stop one
 * record, stop < start none, start or stop <= 0 or above rec_length InvalidIndexRange; sections of
 * different level-1 records never merge.  SIZE: SizePart per part in wrapping int64 over file_size
 * and chunk_size (any value ParseInt accepted, 0 and negatives included); host arithmetic.
 * d_rows (nrows rows, idx_length = TotalUnits) is the index named in the request, d_rec_rows
 * (rec_nrows, rec_length) the node's record index (CHUNK_RANGE only); both 16-byte aligned.
 * Errors: SHOCKIDX_EFORMAT with Go's text (IndexNoFile / InvalidIndexRange / IndexOutBounds),
 * *err_part (optional) = the failing part, else -1; result->count = result->size = 0 and d_secs is
 * undefined.  Go's order of evaluation decides: part k's own parse or bounds error comes before any
 * level-2 error of part k, and both after every error of a part before k.  d_rows == NULL is the
 * missing index file at part 0 (modes 0-2); d_rec_rows == NULL is IndexNoFile at the first part whose
 * level 1 yields a record, and no error when none does.  nparts == 0 succeeds with no sections.
 * A short secs_cap returns SHOCKIDX_ESPACE with result->count = the sections needed, nothing
 * written.  More than 2^20 parts, or more than INT32_MAX rows visited in one level, is
 * SHOCKIDX_EINVAL. */
int shockidx_download_plan(shockidx_ctx *ctx, int mode, const char *const *parts, uint64_t nparts,
                           const void *d_rows, uint64_t nrows, int64_t idx_length,
                           const void *d_rec_rows, uint64_t rec_nrows, int64_t rec_length,
                           int64_t file_size, int64_t chunk_size,
                           void *d_secs, uint64_t secs_cap, int64_t *err_part, shockidx_subset_result *result);

/* ---- chunkrecord index -----------------------------------------
 * Indexers["chunkrecord"] (index/index.go:21-28, index/chunkrecord.go:41-99): rows of ~chunk
 * bytes (conf.CHUNK_SIZE = 1048576 when chunk == 0) ending where fastq.Record's last match in
 * the chunk's final 32 KiB ends (FASTQ) or at the last "\n>" / "\r>" (FASTA); the last row
 * runs to the end of the file.  d_data: n bytes in HBM; d_rows: row_cap rows; at most
 * n / (chunk - 32767) + 2 rows are produced.  fmt AUTO detects like DetermineFormat; a SAM
 * file returns SHOCKIDX_EFORMAT (the reference loops forever there, sam.go:100-102). */
int shockidx_chunkrecord_device(shockidx_ctx *ctx, const void *d_data, uint64_t n, int fmt, uint64_t chunk,
                                void *d_rows, uint64_t row_cap, shockidx_result *result);
/* The same over an open descriptor (not closed; pread from offset 0, short reads retried):
 * *rows receives a malloc'ed table of result->count rows (free with shockidx_free). */
int shockidx_chunkrecord_fd(shockidx_ctx *ctx, int fd, uint64_t n, int fmt, uint64_t chunk, uint64_t **rows,
                            shockidx_result *result);

/* chunkRecord.Create for a subset node whose index format is not "matrix"
 * (index/chunkrecord.go:100-228): the subset node's record index (d_ri: nrows device rows,
 * whole rows only, as its ReadAt loop reads them) grouped into chunks of rows below 1 MiB;
 * d_rows receives result->count rows (16 * first row, 16 * rows): the "matrix" index. */
int shockidx_chunkrecord_subset_device(shockidx_ctx *ctx, const void *d_ri, uint64_t nrows, void *d_rows,
                                       uint64_t row_cap, shockidx_result *result);

/* ---- chunkrecord in slabs ---------------------------------------------------------------------
 * The same table as shockidx_chunkrecord_device built slab by slab, so that the device holds two
 * input slots, one slab's workspace and one slab's rows however large the node is.  SeekChunk
 * (fastq.go:216-243, fasta.go:143-173) reads only 32 KiB windows and the file size, and a window's
 * result depends on its own bytes alone, so a chunk is settled by any slab that holds the windows
 * it evaluates.  What crosses a slab end is chunkrecord.go's loop state (curr and count,
 * chunkrecord.go:54-55) and the recursion state of the one chunk left open: the offSet of
 * SeekChunk's next window (== curr while the chunk's first window, the lastIndex one, has not been
 * evaluated).  The carry holds them with the format and whether the EOF row (chunkrecord.go:60-64)
 * is out.
 *
 * The slab (shockidx_slab): the window is the file bytes [base - front, base + end); d_data, the
 * address of file byte base, is 16-byte aligned (base itself may be any offset); n and seq are
 * ignored; is_first: the walk's first slab, whose window starts at 0 (front == base; a later slab's
 * window may start at 0 too, with is_first 0); is_last: base + end == file_size.
 * Slabs go in file order.  The first one initialises the carry (d_carry:
 * shockidx_chunkrecord_carry_bytes() bytes of device memory, 8-byte aligned: a header and two
 * halves, a slab reads one and writes the other) and resolves fmt: SHOCKIDX_FMT_AUTO needs the
 * first min(32768, file_size) bytes inside the window and byte 0 at a 16-byte-aligned address, else
 * SHOCKIDX_EINVAL; SAM is SHOCKIDX_EFORMAT as in shockidx_chunkrecord_device.  Later slabs take the
 * format from the carry and ignore fmt.  chunk as in shockidx_chunkrecord_device, the same for
 * every slab.
 *
 * A slab emits, at file offsets into d_rows[0 .. count), every row whose windows all lie in its
 * window (chunkrecord.go:65-75), and on the last slab the EOF row.  A window [w, w + 32768) with
 * w + 32768 > base + end is io.EOF on the last slab and "not here" on any other: the walk stops and
 * the carry keeps (curr, offSet).  No byte outside the window is read.
 *
 * Returns: SHOCKIDX_OK, count = the rows written by this call -- possibly 0, when no window of the
 * open chunk lies in the slab (e.g. chunk larger than the slab).  Any other return leaves the carry
 * as it was (the first slab: as it initialised it) and no row that counts: SHOCKIDX_EINVAL, the
 * carry's next window starts before the slab's window, or its walk has already ended;
 * SHOCKIDX_ESPACE, count = the rows the slab needs.  The slabs' rows concatenated are
 * shockidx_chunkrecord_device's table, and after the last slab the carry's count is the table's.
 * Consecutive slabs never fail the carry's precondition when each window starts at most
 * (32768 bytes) before the previous one's end.
 * result->path 6; result->reruns = the speculative rounds of this slab (0 with
 * SHOCKIDX_CHUNK_MODE=serial); result->state_out = 1 once the EOF row is out. */
uint64_t shockidx_chunkrecord_carry_bytes(void);
int shockidx_chunkrecord_slab_device(shockidx_ctx *ctx, const shockidx_slab *slab, uint64_t file_size, int fmt,
                                     uint64_t chunk, void *d_carry, void *d_rows, uint64_t row_cap,
                                     shockidx_result *result);
/* The walk over an open descriptor (chunkrecord.go:41-99 whatever the node's size): slot k holds the
 * file bytes [max(0, k S - 64 KiB), min(n, (k + 1) S)), slab k + 1 crosses PCIe into one slot while
 * slab k is walked in the other, each slab's rows go to the host as they are made.  slab_bytes
 * (S, at least 64 KiB) 0: sized so that the two slots, one slab's workspace and one slab's rows fit
 * the context's device budget (shockidx_ctx_set_dev_cap; under 32 MiB: SHOCKIDX_ENOMEM).  No slab is
 * submitted twice and no input needs a larger slot: the window a walk stops at always lies in the
 * next slot.  *rows receives a malloc'ed table of result->count rows (free with shockidx_free);
 * result->path 6, result->reruns = the speculative rounds of all slabs.  shockidx_chunkrecord_fd
 * takes this walk when the whole-node build (the node, its FASTQ record table or FASTA tile arrays,
 * the graph, the rows) does not fit the budget, and is otherwise unchanged. */
int shockidx_chunkrecord_fd_walk(shockidx_ctx *ctx, int fd, uint64_t n, int fmt, uint64_t chunk, uint64_t slab_bytes,
                                 uint64_t **rows, shockidx_result *result);

/* ---- column index ------------------------------------------------------------------------
 * CreateColumnIndex (index/column.go:33-130, called from node/index.go:43-54 for
 * PUT /node/{id}/index/column?number=N): a tab-separated file grouped by the runs of one
 * column.  Lines are the ReadBytes('\n') pieces (column.go:54); a piece of at most one byte is
 * skipped and its bytes stay with the open group (:64-72); a row ends before every other line
 * whose column-th field (bytes.Split on '\t', :74-79; the last field keeps its "\n") differs
 * from the previous compared line's (:80-98, prev_str starts ""), except at line 0.  Rows are
 * contiguous (offset, length) pairs that cover the file; a file of one group has no rows
 * (:119: curr == 0).  column counts from 1; column < 1 is SHOCKIDX_EINVAL (the controller
 * rejects it, controller/node/index/index.go:218-228).
 * Error: the first non-blank line with fewer than column fields returns SHOCKIDX_EFORMAT,
 * "Specified column does not exist for all lines in file." (:75-77), count 0.  The reference
 * tests len(slices) < column-1, so a line with exactly column-1 fields passes that test and
 * panics at slices[column-1] (:79, index out of range: the server goes down); both cases
 * return the error here.
 * d_data: n bytes in HBM; d_rows: row_cap rows; a short row_cap returns SHOCKIDX_ESPACE with
 * result->count = the rows needed.  result->format is SHOCKIDX_FMT_LINE; result->path is 1 for
 * the tile pass (one read of the input) and 2 for the general build (the line index, then one key
 * per line compared with its predecessor's; SHOCKIDX_COLUMN_MODE=two forces it). */
int shockidx_column_device(shockidx_ctx *ctx, const void *d_data, uint64_t n, int column, void *d_rows,
                           uint64_t row_cap, shockidx_result *result);
/* The same over an open descriptor (not closed; pread from offset 0, short reads retried):
 * *rows receives a malloc'ed table of result->count rows (free with shockidx_free). */
int shockidx_column_fd(shockidx_ctx *ctx, int fd, uint64_t n, int column, uint64_t **rows,
                       shockidx_result *result);

/* ---- column index in slabs ------------------------------------------------------------------
 * The same table built slab by slab, so that the device holds two input slots, one slab's workspace
 * and one slab's rows however large the node is.  column.go's loop carries four things from line
 * to line (column.go:44-48): curr (the open group's start), the rows written, line_count != 0 and
 * prev_str.  A slab takes them from the carry and leaves them in it; nothing else crosses a slab
 * end.
 *
 * The slab (shockidx_slab): d_data 16-byte aligned; n owned bytes, end readable bytes from d_data
 * (n + halo), front readable bytes before it (at least 16 unless base < 16); base, the file offset
 * of d_data[0], may be any offset and n any length; is_first: base == 0; is_last: the owned bytes
 * end the file (base + n == file_size); seq is ignored.  A line belongs to the slab that holds the
 * '\n' before it, the line at offset 0 to the first slab.  Slabs are submitted in file order; the
 * first one initialises the carry (d_carry: shockidx_column_carry_bytes() bytes of device memory,
 * 8-byte aligned, never read by the host: a header and two halves of a state with up to
 * SHOCKIDX_COLUMN_KEYCAP key bytes -- a slab reads one half and writes the other).
 *
 * A slab decides the cut before each non-blank line it owns (column.go:80: its key against the
 * previous non-blank line's, for its first such line the carried key; before any compared line
 * prev_str is "" and the line at offset 0 never cuts, :80,99-101) and writes the row each cut closes,
 * (prev_cut, cut - prev_cut) at file offsets, to d_rows[0 .. count); the last slab also writes the
 * row that runs to file_size when the file has a cut (:119-125).  The slabs' rows concatenated are
 * shockidx_column_device's table.
 *
 * Returns: SHOCKIDX_OK, count = the rows written.  Any other return leaves the carry as it was and
 * no row that counts, so the call may be repeated: SHOCKIDX_ESPACE, count = the rows the slab
 * needs; SHOCKIDX_EFORMAT, the missing-column error (:75-79), count 0 -- the caller drops the rows
 * of earlier slabs, the reference returns none; SHOCKIDX_EMORE, state_out = the file offset of the
 * first owned line the slab cannot settle inside [d_data - front, d_data + end): its key does not
 * close there (for a line with too few fields, or with the key in its last field, its end does
 * not), or it is the last non-blank owned line of a slab that is not the file's last and its key
 * is longer than SHOCKIDX_COLUMN_KEYCAP.  When a line without the column and an unsettled line are
 * both present, the earlier one decides.  No byte outside the window is read.  result->path 5. */
#define SHOCKIDX_COLUMN_KEYCAP 65536
uint64_t shockidx_column_carry_bytes(void);
int shockidx_column_slab_device(shockidx_ctx *ctx, const shockidx_slab *slab, uint64_t file_size, int column,
                                void *d_carry, void *d_rows, uint64_t row_cap, shockidx_result *result);
/* The walk over an open descriptor: slab k + 1 crosses PCIe into one slot while slab k is indexed
 * in the other, each slab's rows go to the host as they are made.  slab_bytes 0: sized so that the
 * slots, the workspace and the rows fit the context's device budget (shockidx_ctx_set_dev_cap, at
 * least 32 MiB); halo_bytes 0: 4 MiB (a sixteenth of a budget under 64 MiB).  SHOCKIDX_EMORE from a
 * slab at offset x: the slab is submitted again as [base, x - 1) and the next one starts at x - 1;
 * when x - 1 is the slab's base, no slot can hold the line or key: SHOCKIDX_ENOMEM.  result->reruns
 * counts the slabs submitted again.  shockidx_column_fd takes this walk when the whole node, its
 * workspace and its rows do not fit the budget. */
int shockidx_column_fd_walk(shockidx_ctx *ctx, int fd, uint64_t n, int column, uint64_t slab_bytes,
                            uint64_t halo_bytes, uint64_t **rows, shockidx_result *result);
/* CreateColumnIndex's file protocol (column.go:36-44,109-129): the table into a temp file under
 * tmpdir, renamed to outpath; a file of one group leaves a zero-byte file.  Within the budget the
 * whole-node build, else the walk, whose rows are written at 16 * row as each slab delivers them.
 * On any error nothing is left at outpath or in tmpdir. */
int shockidx_column_create(shockidx_ctx *ctx, int fd, uint64_t n, int column, const char *tmpdir,
                           const char *outpath, shockidx_result *result);

/* ---- The batch build: many small nodes indexed in one call -----------------------------------
 * A batch is a list of nnodes nodes {int64 pos, int64 len} (the layout of the stream's sections) of
 * one byte arena, both in HBM, with one kind and one fmt (AUTO: detected per node) for all of them.
 * Node i's result is exactly shockidx_build_device's over the bytes [pos, pos + len) alone: count,
 * format, status, Go's error text and the rows, whose offsets are relative to the node's first byte.
 * Nodes are independent: a node in error, or of no detectable format, changes nothing for the
 * others, and no byte outside a node influences its result.  pos must be 16-byte aligned and
 * pos + len <= data_len; anything else is SHOCKIDX_EINVAL for the call with nothing written.
 * d_data and d_rows are 16-byte aligned, d_nodes 8-byte aligned.
 *
 * Rows of node i are d_rows[row_off .. row_off + count); row_off does not decrease along the list
 * and the regions do not overlap (the table is not dense behind a node that ended in an error).
 * *rows_total is the table's extent in rows.  A row_cap below it returns SHOCKIDX_ESPACE with
 * *rows_total = a capacity with which the same call succeeds, and nothing written to d_rows.
 *
 * The call's return code and result->status report system errors only; a format error is per node,
 * in items[i].status, and the call returns SHOCKIDX_OK.  result->count = the nodes with status OK.
 * Nodes of at most SHOCKIDX_BATCH_SMALL bytes (environment, read per call; default 256 KiB; 0: none)
 * are indexed together, in a number of kernel launches and host waits that does not depend on
 * nnodes, on which formats occur or on how they interleave; longer ones go through the single build
 * one at a time, in list order, into their region of the same table (one wave still counts such a
 * node's rows first: a node of hundreds of MiB belongs in shockidx_build_device). */
typedef struct shockidx_batch_item { /* one per node, host memory */
  uint64_t count;     /* rows valid for this node: the records before an error */
  uint64_t row_off;   /* its first row in the batch's table (rows, not bytes) */
  int32_t format;     /* SHOCKIDX_FMT_* indexed (SHOCKIDX_FMT_NONE: none detected) */
  int32_t status;     /* SHOCKIDX_OK or SHOCKIDX_EFORMAT */
  uint32_t term_code; /* device status of the terminating record (diagnostic) */
  uint32_t path;      /* 5: the batched walk; otherwise the single build's path (1, 2) */
  uint64_t err_pos;   /* FASTA: the invalid piece, relative to the node */
  uint64_t err_len;
} shockidx_batch_item;
int shockidx_build_batch_device(shockidx_ctx *ctx, const void *d_data, uint64_t data_len, const void *d_nodes,
                                uint64_t nnodes, int kind, int fmt, void *d_rows, uint64_t row_cap,
                                shockidx_batch_item *items, uint64_t *rows_total, shockidx_result *result);
/* The same over nnodes bodies in host memory: packed into one arena at 16-byte aligned positions
 * (in list order), copied to HBM and indexed.  *rows receives one malloc'ed table (free with
 * shockidx_free); items[i].row_off places node i in it.  The context keeps the packed arena until
 * its next call, for shockidx_batch_error(ctx, NULL, ...). */
int shockidx_build_batch_host(shockidx_ctx *ctx, const void *const *bodies, const uint64_t *lens, uint64_t nnodes,
                              int kind, int fmt, uint64_t **rows, shockidx_batch_item *items,
                              shockidx_result *result);
/* Go's error text for one failed node of the last batch, byte for byte what the single build
 * reports (at most 255 bytes; *len = the bytes written to buf, never more than cap; no NUL is
 * added).  d_data: the arena of the device call, or NULL after shockidx_build_batch_host; node: the
 * node's {int64 pos, int64 len} in host memory (after _host its position in the packed arena:
 * node 0 at 0, each next node at the 16-byte boundary at or after its predecessor's end).  A node
 * whose status is SHOCKIDX_OK has an empty text. */
int shockidx_batch_error(shockidx_ctx *ctx, const void *d_data, const shockidx_batch_item *item, const void *node,
                         char *buf, uint64_t cap, uint64_t *len);
/* How the context's last batch call ran (the results do not depend on it). */
typedef struct shockidx_batch_stats {
  uint64_t nodes;        /* nnodes of the call */
  uint64_t batches;      /* batched walks (0 or 1: every small node, whatever its format) */
  uint64_t batched;      /* nodes inside it */
  uint64_t singles;      /* nodes that went through the single build */
  uint64_t by_format[4]; /* nodes indexed as FASTQ, FASTA, SAM, line */
  uint64_t launches;     /* kernel launches the batched walk made (a single counts as one) */
  uint64_t waits;        /* host waits on the stream (a single adds its build's own) */
} shockidx_batch_stats;
int shockidx_batch_last_stats(const shockidx_ctx *ctx, shockidx_batch_stats *out);

void shockidx_free(void *p);
const char *shockidx_strerror(int code);
int shockidx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SHOCKIDX_H */
