// sidx_chunk_api.cpp -- the chunkrecord entry points of the C ABI (index/chunkrecord.go): the
// serial walk, the speculative build over sidx_chunk.hip, chunkrecord of a subset node, and the
// same table one slab at a time (chunkrecord.go:54-97 with its state in a device carry) for nodes
// that do not fit the device budget.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_chunkwalk.hpp"
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
    HIPCHK(sidx_cr_graph(dd, n, fasta, chunk, base, stride, nb, 0, ft, J1, Ja, Jb, levels, &JL, s), "chunk graph");
    u64 y = 0, k0 = 0;
    for (u64 miss = 0; miss < 64;) {
      ++*rounds;
      HIPCHK(sidx_cr_round(dd, n, fasta, chunk, base, stride, nb, 0, ft, JL, J1, 1u << levels, y, k0, cap, heads, pos,
                           mres, ctl, rows, row_cap, c->cr_grid, 0, s),
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

// ---- the slab step ---------------------------------------------------------------------------
bool chunk_serial_mode() {
  const char *mode = getenv("SHOCKIDX_CHUNK_MODE");
  return mode && !strcmp(mode, "serial");
}
u64 *slab_st(shockidx_ctx *c) { return (u64 *)(c->d_small + SMALL_CHUNK); }
static_assert(SMALL_CHUNK + CRS_WORDS * sizeof(u64) <= SMALL_SLABSUM, "small layout");

// the slab step's control words, waited for
int read_st(shockidx_ctx *c, hipStream_t s, u64 h[CRS_WORDS], Err res) {
  HIPCHK(hipMemcpyAsync(c->h_det, slab_st(c), CRS_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s), "chunk slab copy");
  HIPCHK(hipStreamSynchronize(s), "chunk slab sync");
  memcpy(h, c->h_det, CRS_WORDS * sizeof(u64));
  return 0;
}

// file offsets of the view whose device address is 16-byte aligned: the last one <= x, the first >= x
u64 addr_dn(const ChunkView &v, u64 x) { return x - (((uintptr_t)v.d - v.lo + x) & 15); }
u64 addr_up(const ChunkView &v, u64 x) { return x + ((16 - (((uintptr_t)v.d - v.lo + x) & 15)) & 15); }

ChunkWalkDev walk_dev(shockidx_ctx *c, u64 len) {
  size_t sb = 0;
  (void)sidx_cr_gpos_count(nullptr, len, nullptr, nullptr, nullptr, nullptr, &sb, c->stream);
  return ChunkWalkDev{(sizeof(ChunkCarry) + 255) & ~255ull, sb, sidx_cr_gslot(), c->tiles_grid};
}

// The speculative build over a view, from the start y0 of a chunk whose first window is still to
// come, k0 rows of this slab out: node positions from the view alone (predictions: a record index
// of the view's bytes from an aligned offset at or after y0 with a guessed line phase for FASTQ,
// the view's "\n>" positions for FASTA, each behind node 0 = y0), the graph, then rounds of path +
// exact evaluation as chunk_spec.  A round ends at a chunk whose window the view does not hold
// (the path's last when the path holds): *y = that chunk's start, *k = the rows before it.
// *final: a serial step in between already reached the view's end (the state is in the control
// words).  The tables are capped by the view's length (sidx_chunkwalk.hpp), never grown.
int chunk_slab_spec(shockidx_ctx *c, const ChunkView &v, int fasta, u64 chunk, u64 *rows, u64 row_cap, hipStream_t s,
                    u64 *y, u64 *k, bool *final, u64 *rounds, shockidx_result *res) {
  constexpr u64 CT = CHUNKWALK_CT;
  *final = false;
  const u64 vlen = v.hi - v.lo, y0 = *y;
  const u64 from = y0 > v.lo ? y0 : v.lo;
  const u64 ncap = chunkwalk_nodes_cap(vlen);
  const uint8_t *origin = v.d - v.lo;
  const ChunkWalkDev dv = walk_dev(c, vlen);
  if (int rc = c->d_cra.ensure(chunkwalk_cra_bytes(vlen, dv.scan_bytes, dv.gslot), res)) return rc;
  if (int rc = c->d_crb.ensure(chunkwalk_crb_bytes(vlen, chunk), res)) return rc;
  Carver cv{c->d_crb};
  u64 nb = 0, stride = 1;
  const u64 *base = nullptr;
  if (!fasta) {
    // (the nodes of a record at p are p, p - 1, p - 2: from + 2 on, none lies before the view or y0)
    u64 p0 = from ? addr_up(v, from + 2) : addr_up(v, 0);
    if (p0 && p0 - v.lo < 16) p0 += 16;  // (a slab that is not the file's start looks at the byte before it)
    u64 *tab = c->d_cra.as<u64>();
    u64 got = 0;
    if (p0 < v.hi) {
      u64 guess = 0;
      if (p0) {
        u64 *d_out = (u64 *)(c->d_small + SMALL_DETECT + 32);
        HIPCHK(sidx_launch_slab_guess(origin + p0, v.hi - p0, p0 - v.lo, F_FASTQ, d_out, s), "guess launch");
        HIPCHK(hipMemcpyAsync(c->h_det + 2, d_out, 8, hipMemcpyDeviceToHost, s), "guess copy");
        HIPCHK(hipStreamSynchronize(s), "guess sync");
        memcpy(&guess, c->h_det + 2, 8);
      }
      SlabGeom g;
      g.n = g.end = v.hi - p0;
      g.front = p0 - v.lo;
      g.base = p0;
      g.state_in = guess;
      g.row_base = p0 ? 1 : 0;
      g.eof = v.last;
      g.file_start = p0 == 0;
      g.d_summary = c->d_small + SMALL_SLABSUM;
      DevResult dr;
      shockidx_result r2;
      reset_result(&r2);
      if (int rc = run_index(c, origin + p0, v.hi - p0, F_FASTQ, tab + 2, ncap, s, &dr, &r2, &g)) return forward_error(res, r2, rc);
      if (!(dr.flags & RF_INTERNAL)) got = dr.count > g.row_base ? dr.count - g.row_base : 0;
      if (got > ncap) got = ncap;
    }
    HIPCHK(sidx_cr_slab_nodes(tab, 1, 2, 0, y0, s), "chunk nodes");
    nb = got + 1;
    base = tab;
    stride = 2;
  } else {
    u64 a0 = addr_dn(v, from);
    if (a0 < v.lo) a0 += 16;
    const u64 len = a0 < v.hi ? v.hi - a0 : 0, nt = (len + CT - 1) / CT;
    size_t sb = dv.scan_bytes;
    Carver ca{c->d_cra};
    u64 *tcnt = ca.take<u64>(nt + 1), *toff = ca.take<u64>(nt + 1);
    uint16_t *slot = ca.take<uint16_t>(dv.gslot * (nt + 1));
    void *tmp = ca.take<uint8_t>(sb);
    u64 last[2] = {0, 0};
    if (nt) {
      HIPCHK(sidx_cr_gpos_count(origin + a0, len, tcnt, toff, slot, tmp, &sb, s), "node count");
      HIPCHK(hipMemcpyAsync(c->h_det, toff + nt - 1, 8, hipMemcpyDeviceToHost, s), "node count copy");
      HIPCHK(hipMemcpyAsync((u64 *)c->h_det + 1, tcnt + nt - 1, 8, hipMemcpyDeviceToHost, s), "node count copy");
      HIPCHK(hipStreamSynchronize(s), "node count sync");
      memcpy(last, c->h_det, 16);
    }
    nb = 1 + last[0] + last[1];
    if (nb > ncap + 1) {  // more "\n>" than the table holds: no predictions, the walk alone
      nb = 0;
    } else {
      u64 *G = cv.take<u64>(nb);
      HIPCHK(hipMemsetAsync(G, 0, 8, s), "node 0");
      if (nt) HIPCHK(sidx_cr_gpos_write(origin + a0, len, tcnt, toff, slot, G, s), "node positions");
      HIPCHK(sidx_cr_slab_nodes(G, nb, 1, a0, y0, s), "chunk nodes");
      base = G;
    }
  }
  if (!nb) return 0;  // (*y, *k) as they came: the caller's walk does the slab
  const u64 nn = fasta ? nb : 3 * nb, ntile = vlen / CT + 1;
  const u64 est = (v.hi - from) / chunk + 1, cap = chunkwalk_path_cap(vlen, chunk);
  u64 *ft = cv.take<u64>(ntile + 2);
  u32 *J1 = cv.take<u32>(nn), *Ja = cv.take<u32>(nn), *Jb = cv.take<u32>(nn);
  u32 *heads = cv.take<u32>(cap);
  u64 *pos = cv.take<u64>(cap);
  i64 *mres = cv.take<i64>(cap);
  u64 *ctl = cv.take<u64>(8);
  int levels = 0;
  while (levels < 16 && (est >> levels) > 128) ++levels;
  const u32 *JL = J1;
  HIPCHK(sidx_cr_graph(origin, v.hi, fasta, chunk, base, stride, nb, v.lo, ft, J1, Ja, Jb, levels, &JL, s), "chunk graph");
  u64 yy = y0, k0 = *k;
  for (u64 miss = 0; miss < 64;) {
    ++*rounds;
    HIPCHK(sidx_cr_round(origin, v.hi, fasta, chunk, base, stride, nb, v.lo, ft, JL, J1, 1u << levels, yy, k0, cap, heads,
                         pos, mres, ctl, rows, row_cap, c->cr_grid, 1, s),
           "chunk round");
    HIPCHK(hipMemcpyAsync(c->h_det, ctl, 5 * sizeof(u64), hipMemcpyDeviceToHost, s), "chunk round copy");
    HIPCHK(hipStreamSynchronize(s), "chunk round sync");
    u64 r[5];
    memcpy(r, c->h_det, sizeof r);
    if (r[1] == 0xFFFFFFFDull) {  // not a node: a few exact steps, then the path again
      HIPCHK(sidx_cr_slab_walk(&v, fasta, chunk, slab_st(c), rows, row_cap, 2, 1, yy, k0, s), "chunk walk");
      u64 h[CRS_WORDS];
      if (int rc = read_st(c, s, h, res)) return rc;
      if (h[CRS_STOP]) { *final = true; return 0; }
      yy = h[CRS_CURR];
      k0 = h[CRS_ROWS];
      ++miss;
      continue;
    }
    const bool open = r[2] == ~0ull || (i64)r[3] < 0;  // the round ends at a chunk the view cannot close
    if (open) {
      k0 += r[2] == ~0ull ? r[0] - 1 : r[2];
      yy = r[4];
      break;
    }
    if (!(r[1] == 0xFFFFFFFCull && r[2] + 1 == r[0])) ++miss;  // not just the path's capacity
    yy = r[4];
    k0 += r[2] + 1;
  }
  *y = yy;
  *k = k0;
  return 0;
}

}  // namespace

namespace sidx_host {

u64 chunk_one_pass_bytes(shockidx_ctx *c, u64 n, u64 chunk) { return chunkwalk_whole_bytes(n, chunk, walk_dev(c, n)); }
ChunkWalkDev chunk_walk_dev(shockidx_ctx *c, u64 len) { return walk_dev(c, len); }

// One slab: the carry into the control words (one host stop: the format and where the walk stands),
// the open chunk's remaining windows by the serial evaluator, the speculative build from there
// (or the serial walk: SHOCKIDX_CHUNK_MODE=serial, a view that cannot hold the next chunk's first
// window), the serial walk again for the chunk the view leaves open or the EOF row, and -- only
// when the rows fit -- the end state into the carry's other half.
int chunk_slab_run(shockidx_ctx *c, const ChunkView &v, u64 chunk, bool first, int fmt, ChunkCarry *carry, u64 *rows,
                   u64 row_cap, hipStream_t s, shockidx_result *res) {
  res->path = 6;
  u64 *st = slab_st(c);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(sidx_cr_slab_begin(&v, chunk, first, fmt, carry, st, s), "chunk slab launch");
  u64 h[CRS_WORDS];
  if (int rc = read_st(c, s, h, res)) return rc;
  res->format = (int)h[CRS_FMT];
  if (h[CRS_STATUS] == CRS_BEFORE) return set_msg(res, SHOCKIDX_EINVAL, "chunkrecord slab: the carry's next window starts before the slab's window");
  if (h[CRS_STATUS] != CRS_OK) return set_msg(res, SHOCKIDX_EINVAL, "chunkrecord slab: the carry's walk has ended");
  const int fasta = h[CRS_FMT] == SHOCKIDX_FMT_FASTA;
  u64 rounds = 0;
  bool walked = false;
  if (!chunk_serial_mode()) {
    bool stop = false;
    if (h[CRS_OFF] > h[CRS_CURR]) {  // mid-chunk: that chunk first, by the serial evaluator
      HIPCHK(sidx_cr_slab_walk(&v, fasta, chunk, st, rows, row_cap, 1, 0, 0, 0, s), "chunk walk");
      if (int rc = read_st(c, s, h, res)) return rc;
      stop = h[CRS_STOP] != 0;
      walked = stop;
    }
    if (!stop && h[CRS_CURR] + chunk <= v.hi) {
      u64 y = h[CRS_CURR], k = h[CRS_ROWS];
      bool final = false;
      if (int rc = chunk_slab_spec(c, v, fasta, chunk, rows, row_cap, s, &y, &k, &final, &rounds, res)) return rc;
      if (!final) HIPCHK(sidx_cr_slab_walk(&v, fasta, chunk, st, rows, row_cap, ~0ull, 1, y, k, s), "chunk walk");
      walked = true;
    }
  }
  if (!walked) HIPCHK(sidx_cr_slab_walk(&v, fasta, chunk, st, rows, row_cap, ~0ull, 0, 0, 0, s), "chunk walk");
  if (int rc = read_st(c, s, h, res)) return rc;
  res->reruns = (uint32_t)rounds;
  res->count = h[CRS_ROWS];
  if (h[CRS_ROWS] > row_cap) return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  HIPCHK(sidx_cr_slab_commit(carry, st, s), "chunk carry launch");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipEventSynchronize(c->ek1), "event sync");
  float kms = 0.f;
  (void)hipEventElapsedTime(&kms, c->ek0, c->ek1);
  res->kernel_ms = res->index_ms = kms;
  res->state_out = h[CRS_DONE];
  return SHOCKIDX_OK;
}

}  // namespace sidx_host

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
  // a node whose whole-node build does not fit the device budget goes through two slab slots
  if (chunk_one_pass_bytes(c, n, chunk) > dev_budget(c)) return shockidx_chunkrecord_fd_walk(c, fd, n, fmt, chunk, 0, rows, res);
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

uint64_t shockidx_chunkrecord_carry_bytes(void) { return sizeof(ChunkCarry); }

// One slab of chunkrecord (chunkrecord.go:54-97 with its loop state, and the state of the one
// SeekChunk recursion a slab end can cut, carried from slab to slab).
int shockidx_chunkrecord_slab_device(shockidx_ctx *c, const shockidx_slab *slab, uint64_t file_size, int fmt,
                                     uint64_t chunk, void *d_carry, void *d_rows, uint64_t row_cap, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  res->path = 6;
  if (!chunk) chunk = 1048576;
  if (!c || !slab || !d_carry || (!d_rows && row_cap) || chunk < 32768 || chunk > (1ull << 40))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const shockidx_slab &b = *slab;
  // (a later slab's window may start at 0 too: is_first names the walk's first slab, not the offset)
  const bool first = b.is_first != 0, last = b.end <= file_size && b.base == file_size - b.end;
  if (b.front > b.base || b.base > file_size || b.end > file_size - b.base || (b.front + b.end && !b.d_data) ||
      ((uintptr_t)b.d_data & 15) || (first && b.front != b.base) || (b.is_last != 0) != last || ((uintptr_t)d_carry & 7))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const ChunkView v{(const uint8_t *)b.d_data - b.front, b.base - b.front, b.base + b.end, file_size, last};
  int kfmt = 0;
  if (first) {  // the first slab resolves the format (later ones take it from the carry)
    const u64 need = file_size < 32768 ? file_size : 32768;
    if (fmt == SHOCKIDX_FMT_AUTO && (v.hi < need || ((uintptr_t)v.d & 15)))
      return set_msg(res, SHOCKIDX_EINVAL, "chunkrecord slab: format detection needs the file's first 32 KiB in the first slab");
    if (int rc = resolve_format(c, v.d, v.hi, SHOCKIDX_RECORD, fmt, s, &kfmt, res)) return rc;
    res->format = kfmt;
    if (kfmt == SHOCKIDX_FMT_SAM)
      return set_msg(res, SHOCKIDX_EFORMAT, "chunkrecord: sam.SeekChunk never advances (reference loops forever)");
    if (kfmt != SHOCKIDX_FMT_FASTA && kfmt != SHOCKIDX_FMT_FASTQ) return set_msg(res, SHOCKIDX_EINVAL, "invalid format");
  }
  const int rc = chunk_slab_run(c, v, chunk, first, kfmt, (ChunkCarry *)d_carry, (u64 *)d_rows, row_cap, s, res);
  res->total_ms = now_ms() - t0;
  return rc;
}

// The slab walk over an open descriptor, whatever the node's size: the table back to a malloc'ed
// array (result->path 6).
int shockidx_chunkrecord_fd_walk(shockidx_ctx *c, int fd, uint64_t n, int fmt, uint64_t chunk, uint64_t slab_bytes,
                                 uint64_t **rows, shockidx_result *res) {
  shockidx_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !rows || fd < 0) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *rows = nullptr;
  if (!chunk) chunk = 1048576;
  if (chunk < 32768 || chunk > (1ull << 40) || (slab_bytes && slab_bytes < 65536))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  const u64 est = n / (chunk - 32767) + 2;  // (the sink is sized in input bytes, a row per 32, and grows past that)
  TableSink sink(32 * (est < (1ull << 22) ? est : (1ull << 22)));
  if (!sink.out) return set_msg(res, SHOCKIDX_ENOMEM, "out of host memory");
  if (int rc = chunk_fd_walk(c, fd, n, fmt, chunk, slab_bytes, sink, res)) return rc;
  *rows = (uint64_t *)sink.out;
  sink.out = nullptr;
  return SHOCKIDX_OK;
}

}  // extern "C"
