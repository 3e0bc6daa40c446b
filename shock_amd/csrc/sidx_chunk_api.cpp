// sidx_chunk_api.cpp -- the chunkrecord entry points of the C ABI (index/chunkrecord.go): the
// serial walk, the speculative build over sidx_chunk.hip, and chunkrecord of a subset node.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_subset.hpp"
#include "sidx_launch.hpp"
#include "sidx_host.hpp"

using namespace sidx;
using namespace sidx_host;

namespace {

// The serial walk from (curr, cnt) for at most `steps` chunks (UINT64_MAX: to the end)
int chunk_serial(shockidx_ctx *c, const uint8_t *dd, u64 n, int fasta, u64 chunk, u64 *rows, u64 row_cap,
                 u64 curr, u64 cnt, u64 steps, hipStream_t s, u64 out[3], Err res) {
  u64 *d_out = (u64 *)(c->d_small + SMALL_CHUNK);
  HIPCHK(sidx_launch_chunkrecord(dd, n, fasta, (long long)chunk, rows, row_cap, d_out, (long long)curr, cnt, steps, s),
         "chunkrecord launch");
  HIPCHK(hipMemcpyAsync(c->h_det, d_out, 3 * sizeof(u64), hipMemcpyDeviceToHost, s), "chunkrecord copy");
  HIPCHK(hipStreamSynchronize(s), "chunkrecord sync");
  memcpy(out, c->h_det, 3 * sizeof(u64));
  return 0;
}

// Speculative chunkrecord (sidx_chunk.hip): predicted-successor graph over the node positions,
// its jump table, then rounds of path + exact evaluation of every chunk on the path; a chunk
// whose exact successor differs re-enters the path there (or a few serial steps first when
// that position is not a node).  *count = rows of the serial definition.
int chunk_spec(shockidx_ctx *c, const uint8_t *dd, u64 n, int kfmt, u64 chunk, u64 *rows, u64 row_cap,
               hipStream_t s, u64 *count, u64 *rounds, Err res) {
  const int fasta = kfmt == SHOCKIDX_FMT_FASTA;
  constexpr u64 CT = 16384;
  // rows of the path per round: about the chunk count (chunks average between chunk - 32 KiB
  // and chunk bytes); a longer file takes further rounds
  const u64 ntile = n / CT + 1, est = n / chunk + 1, cap = 2 * est + 1024;
  u64 nb = 0, stride = 1;
  const u64 *base = nullptr;
  const u64 *toff_g = nullptr, *tcnt_g = nullptr;  // FASTA: per-tile node counts, their offsets
  const uint16_t *slot_g = nullptr;                 //   and the tiles' kept positions
  auto carve = [](uint8_t *&q, u64 bytes) { uint8_t *r = q; q += (bytes + 255) & ~255ull; return r; };
  if (!fasta) {  // the FASTQ record index (valid up to its first error) gives the node positions
    u64 rcap = n / 128 + 4096;
    for (int attempt = 0; attempt < 2; ++attempt) {
      if (int rc = c->d_cra.ensure(rcap * 16, res)) return rc;
      DevResult dr;
      shockidx_result r2;
      reset_result(&r2);
      if (int rc = run_index(c, dd, n, F_FASTQ, c->d_cra.as<u64>(), rcap, s, &dr, &r2)) return forward_error(res, r2, rc);
      nb = dr.count;
      if (dr.flags & RF_CAPACITY) { rcap = dr.count + 1; nb = 0; continue; }
      break;
    }
    base = c->d_cra.as<u64>();
    stride = 2;
    if (nb && (3 * nb >= 0xFFFFFFF0ull)) nb = 0;
  } else {  // FASTA: every '>' preceded by '\n', plus position 0
    const u64 nt = (n + CT - 1) / CT;
    size_t sb = 0;
    HIPCHK(sidx_cr_gpos_count(dd, n, nullptr, nullptr, nullptr, nullptr, &sb, s), "scan size");
    const u64 slot_bytes = 2ull * sidx_cr_gslot() * nt;
    if (int rc = c->d_cra.ensure(16 * nt + slot_bytes + sb + 2048, res)) return rc;
    uint8_t *q = c->d_cra;
    u64 *tcnt = (u64 *)carve(q, 8 * nt), *toff = (u64 *)carve(q, 8 * nt);
    uint16_t *slot = (uint16_t *)carve(q, slot_bytes);
    toff_g = toff;
    tcnt_g = tcnt;
    slot_g = slot;
    HIPCHK(sidx_cr_gpos_count(dd, n, tcnt, toff, slot, q, &sb, s), "node count");
    u64 last[2] = {0, 0};
    if (nt) {
      HIPCHK(hipMemcpyAsync(c->h_det, toff + nt - 1, 8, hipMemcpyDeviceToHost, s), "node count copy");
      HIPCHK(hipMemcpyAsync((u64 *)c->h_det + 1, tcnt + nt - 1, 8, hipMemcpyDeviceToHost, s), "node count copy");
      HIPCHK(hipStreamSynchronize(s), "node count sync");
      memcpy(last, c->h_det, 16);
    }
    nb = 1 + last[0] + last[1];
    if (nb >= 0xFFFFFFF0ull) nb = 0;
  }
  const u64 nn = fasta ? nb : 3 * nb;
  if (nb) {
    const u64 need = (fasta ? 8 * nb : 0) + 8 * (ntile + 2) + 12 * nn + 4 * cap + 16 * cap + 64 + 16 * 256;
    if (int rc = c->d_crb.ensure(need, res)) return rc;
    uint8_t *q = c->d_crb;
    if (fasta) {
      u64 *G = (u64 *)carve(q, 8 * nb);
      HIPCHK(hipMemsetAsync(G, 0, 8, s), "node 0");
      HIPCHK(sidx_cr_gpos_write(dd, n, tcnt_g, toff_g, slot_g, G, s), "node positions");
      base = G;
    }
    u64 *ft = (u64 *)carve(q, 8 * (ntile + 2));
    u32 *J1 = (u32 *)carve(q, 4 * nn), *Ja = (u32 *)carve(q, 4 * nn), *Jb = (u32 *)carve(q, 4 * nn);
    u32 *heads = (u32 *)carve(q, 4 * cap);
    u64 *pos = (u64 *)carve(q, 8 * cap);
    i64 *mres = (i64 *)carve(q, 8 * cap);
    u64 *ctl = (u64 *)carve(q, 64);
    int levels = 0;
    while (levels < 16 && (est >> levels) > 128) ++levels;
    const u32 *JL = J1;
    HIPCHK(sidx_cr_graph(dd, n, fasta, chunk, base, stride, nb, ft, J1, Ja, Jb, levels, &JL, s), "chunk graph");
    u64 y = 0, k0 = 0;
    for (u64 miss = 0; miss < 64;) {
      ++*rounds;
      HIPCHK(sidx_cr_round(dd, n, fasta, chunk, base, stride, nb, ft, JL, J1, 1u << levels, y, k0, cap, heads, pos,
                           mres, ctl, rows, row_cap, c->cr_grid, s),
             "chunk round");
      HIPCHK(hipMemcpyAsync(c->h_det, ctl, 5 * sizeof(u64), hipMemcpyDeviceToHost, s), "chunk round copy");
      HIPCHK(hipStreamSynchronize(s), "chunk round sync");
      u64 r[5];
      memcpy(r, c->h_det, sizeof r);
      if (r[1] == 0xFFFFFFFDull) {  // not a node: a few exact steps, then the path again
        u64 o[3];
        if (int rc = chunk_serial(c, dd, n, fasta, chunk, rows, row_cap, y, k0, 2, s, o, res)) return rc;
        if (o[2]) { *count = o[0]; return 0; }
        y = o[1];
        k0 = o[0];
        ++miss;
        continue;
      }
      if (r[2] == ~0ull) { *count = k0 + r[0]; return 0; }  // the whole path holds
      if ((i64)r[3] < 0) { *count = k0 + r[2] + 1; return 0; }  // that chunk is the last
      if (!(r[1] == 0xFFFFFFFCull && r[2] + 1 == r[0])) ++miss;  // not just the path's capacity
      y = r[4];
      k0 += r[2] + 1;
    }
    u64 o[3];  // still disagreeing: walk the rest
    if (int rc = chunk_serial(c, dd, n, fasta, chunk, rows, row_cap, y, k0, ~0ull, s, o, res)) return rc;
    *count = o[0];
    return 0;
  }
  u64 o[3];  // no nodes (e.g. the FASTQ record index fails at record 0): the serial walk
  if (int rc = chunk_serial(c, dd, n, fasta, chunk, rows, row_cap, 0, 0, ~0ull, s, o, res)) return rc;
  *count = o[0];
  return 0;
}

}  // namespace

extern "C" {

// chunkrecord (index/chunkrecord.go:41-99).  Default: the speculative build (chunk_spec);
// SHOCKIDX_CHUNK_MODE=serial: the serial walk alone (the definition, kept as a tested path).
int shockidx_chunkrecord_device(shockidx_ctx *c, const void *d_data, uint64_t n, int fmt, uint64_t chunk,
                                void *d_rows, uint64_t row_cap, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!chunk) chunk = 1048576;  // conf.CHUNK_SIZE (conf/conf.go:138)
  if (!c || (!d_data && n) || (!d_rows && row_cap) || chunk < 32768 || chunk > (1ull << 40))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const uint8_t *dd = (const uint8_t *)d_data;
  int kfmt = 0;
  if (int rc = resolve_format(c, dd, n, SHOCKIDX_RECORD, fmt, s, &kfmt, res)) return rc;
  res->format = kfmt;
  if (kfmt == SHOCKIDX_FMT_SAM)  // sam.SeekChunk returns (0, nil): the Go driver never ends
    return set_msg(res, SHOCKIDX_EFORMAT, "chunkrecord: sam.SeekChunk never advances (reference loops forever)");
  if (kfmt != SHOCKIDX_FMT_FASTA && kfmt != SHOCKIDX_FMT_FASTQ) return set_msg(res, SHOCKIDX_EINVAL, "invalid format");
  const char *mode = getenv("SHOCKIDX_CHUNK_MODE");
  const bool serial = mode && !strcmp(mode, "serial");
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  u64 cnt = 0, rounds = 0;
  if (serial) {
    u64 o[3];
    if (int rc = chunk_serial(c, dd, n, kfmt == SHOCKIDX_FMT_FASTA, chunk, (u64 *)d_rows, row_cap, 0, 0, ~0ull, s, o,
                              res))
      return rc;
    cnt = o[0];
  } else if (int rc = chunk_spec(c, dd, n, kfmt, chunk, (u64 *)d_rows, row_cap, s, &cnt, &rounds, res)) {
    return rc;
  }
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipEventSynchronize(c->ek1), "event sync");
  float kms = 0.f;
  (void)hipEventElapsedTime(&kms, c->ek0, c->ek1);
  res->kernel_ms = res->index_ms = kms;
  res->reruns = rounds;
  res->count = cnt;
  res->total_ms = now_ms() - t0;
  if (cnt > row_cap) return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  return SHOCKIDX_OK;
}

// chunkrecord of a subset node (index/chunkrecord.go:100-228): its record index rows (device,
// R rows) grouped into chunks of rows (sidx_chunk.hip): prefix sums of the lengths, every fresh
// start's successor, the jump table, the path from row 0.  Rows (16 * first row, 16 * rows).
int shockidx_chunkrecord_subset_device(shockidx_ctx *c, const void *d_ri, uint64_t nrows, void *d_rows,
                                       uint64_t row_cap, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || (!d_ri && nrows) || (!d_rows && row_cap)) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  if (nrows >= 0xFFFFFFF0ull) return set_msg(res, SHOCKIDX_EINVAL, "record index too large");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const u64 R = nrows;
  size_t sb = 0;
  HIPCHK(sidx_crs_scan(nullptr, R, nullptr, nullptr, nullptr, &sb, s), "scan size");
  auto r256 = [](u64 b) { return (b + 255) & ~255ull; };
  const u64 need = r256(8 * R + 8) + r256(8 * (R + 1)) + 3 * r256(4 * (R + 1)) + r256(4 * (R + 2)) + 256 + r256(sb);
  if (int rc = c->d_crb.ensure(need, res)) return rc;
  uint8_t *q = c->d_crb;
  auto carve = [&](u64 bytes) { uint8_t *r = q; q += r256(bytes); return r; };
  u64 *len = (u64 *)carve(8 * R + 8), *P = (u64 *)carve(8 * (R + 1));
  u32 *J1 = (u32 *)carve(4 * (R + 1)), *Ja = (u32 *)carve(4 * (R + 1)), *Jb = (u32 *)carve(4 * (R + 1));
  u32 *heads = (u32 *)carve(4 * (R + 2));
  u64 *ctl = (u64 *)carve(256);
  void *scan_tmp = carve(sb);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(sidx_crs_scan((const u64 *)d_ri, R, len, P, scan_tmp, &sb, s), "prefix sums");
  HIPCHK(hipMemcpyAsync(c->h_det, P + R, 8, hipMemcpyDeviceToHost, s), "total copy");
  HIPCHK(hipStreamSynchronize(s), "total sync");
  u64 total = 0;
  memcpy(&total, c->h_det, 8);
  // chunks <= 2 * total / 1 MiB + 2 (a chunk and the row that closes it reach 1 MiB together)
  const u64 est = 2 * (total / 1048576) + 2;
  int levels = 0;
  while (levels < 16 && (est >> levels) > 128) ++levels;
  HIPCHK(sidx_crs_build(P, R, J1, Ja, Jb, levels, heads, (u64 *)d_rows, row_cap, ctl, s), "chunk build");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipMemcpyAsync(c->h_det, ctl, 8, hipMemcpyDeviceToHost, s), "count copy");
  HIPCHK(hipStreamSynchronize(s), "count sync");
  u64 cnt = 0;
  memcpy(&cnt, c->h_det, 8);
  float kms = 0.f;
  (void)hipEventElapsedTime(&kms, c->ek0, c->ek1);
  res->kernel_ms = res->index_ms = kms;
  res->count = cnt;
  res->total_ms = now_ms() - t0;
  if (cnt > row_cap) return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  return SHOCKIDX_OK;
}

// chunkrecord over an open file: every byte to HBM through the pinned pread staging (the
// speculative device walk may inspect any window), the table back to a malloc'ed array
int shockidx_chunkrecord_fd(shockidx_ctx *c, int fd, uint64_t n, int fmt, uint64_t chunk, uint64_t **rows,
                            shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !rows || fd < 0) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  if (!chunk) chunk = 1048576;
  TrimGuard trim{c};
  if (chunk < 32768 || chunk > (1ull << 40)) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  if (int rc = stage_fd(c, fd, 0, n, c->stream, res)) return rc;
  const u64 cap = n / (chunk - 32767) + 2;
  if (int rc = c->d_rows.ensure(cap, res)) return rc;
  const double h2d = res->h2d_ms;
  int rc = shockidx_chunkrecord_device(c, c->d_in, n, fmt, chunk, c->d_rows, c->d_rows.cap, res);
  res->h2d_ms = h2d;
  if (rc != SHOCKIDX_OK) return rc;
  if (int rc2 = fetch_rows(c, res->count, c->stream, rows, res)) return rc2;
  res->total_ms = now_ms() - t0;
  return SHOCKIDX_OK;
}

}  // extern "C"
