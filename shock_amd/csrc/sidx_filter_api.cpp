// sidx_filter_api.cpp -- the download filters of the C ABI (node/filter/: fq2fa, anonymize) over
// the kernels of sidx_filter.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_filtwalk.hpp"
#include "sidx_subset.hpp"
#include "sidx_launch.hpp"
#include "sidx_host.hpp"

using namespace sidx;
using namespace sidx::filt_ctl;
using namespace sidx_host;

namespace {

// The output offsets of K delivered items (the exclusive scan of their lengths) and the bytes
// they take together, waited for; K = 0: nothing is launched.
int scan_lengths(shockidx_ctx *c, const u64 *len, u64 *off, u64 K, void *tmp, size_t *tmp_bytes, u64 *total, Err res) {
  *total = 0;
  if (!K) return 0;
  HIPCHK(sidx_scan_u64(len, off, K, tmp, tmp_bytes, c->stream), "scan");
  return scan_total(c, off, len, K, total, res);
}

// anonymize over a FASTA or SAM section (anonymize.go:28-56 through multi.Reader): the stream
// Read + Format deliver (sidx_filter.hip), count / size delivered, Read's error text.
// size_only: see filter_section.
int anonymize_other(shockidx_ctx *c, const uint8_t *dd, u64 n, int kfmt, uint8_t *d_out, u64 out_cap,
                    shockidx_subset_result *res, double t0, bool size_only) {
  hipStream_t s = c->stream;
  const bool fasta = kfmt == SHOCKIDX_FMT_FASTA;
  u64 K = 0;            // FASTA: boundaries (sequences before the EOF one); SAM: lines
  const u64 *B = nullptr;  // FASTA boundary positions / SAM line rows
  shockidx_result br;
  reset_result(&br);
  size_t tb = 0;
  u64 bstride = 1;  // B[k * bstride]
  bool indexed = false;
  if (fasta && n && !getenv("SHOCKIDX_ANON_SCAN")) {
    // Read's boundaries are the record index's (a '>' with a '\n' since the previous '>',
    // fasta.go:100-138); when the index builds without error they are its row starts 1..R-1,
    // found by the FASTA tile pass in one read.  Otherwise (the index validates pieces Read does
    // not) they come from the unvalidated scan below.
    const int brc = build_resident(c, dd, n, SHOCKIDX_RECORD, SHOCKIDX_FMT_FASTA, s, &br);
    if (brc < 0) return forward_error(res, br, brc);
    if (brc == SHOCKIDX_OK) {
      indexed = true;
      res->kernel_ms += br.kernel_ms;
      K = br.count ? br.count - 1 : 0;
      B = c->d_rows + 2;
      bstride = 2;
      HIPCHK(sidx_scan_u64(nullptr, nullptr, K ? K : 1, nullptr, &tb, s), "scan size");
      if (int rc = c->d_sub.ensure(8 * (K + 1) + 48 * (K + 1) + tb + 4096, res)) return rc;
      HIPCHK(hipEventRecord(c->ek0, s), "event");
    }
  }
  if (fasta && !indexed) {
    const u64 nt = (n + TILE - 1) / TILE;
    size_t fb = 0;
    HIPCHK(sidx_fa_bnd_count(dd, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &fb, s),
           "scan size");
    const u64 slot_bytes = 2ull * sidx_fa_slot() * (nt + 1);
    const u64 need = 6 * 8 * (nt + 1) + slot_bytes + fb + 8 * 256;
    if (int rc = c->d_cra.ensure(need, res)) return rc;
    Carver cv{c->d_cra};
    u64 *lnl = cv.take<u64>(nt + 1), *lgt = cv.take<u64>(nt + 1), *cnl = cv.take<u64>(nt + 1);
    u64 *cgt = cv.take<u64>(nt + 1), *tcnt = cv.take<u64>(nt + 1), *toff = cv.take<u64>(nt + 1);
    uint16_t *slot = cv.take<uint16_t>(sidx_fa_slot() * (nt + 1));
    void *tmp = cv.take<uint8_t>(fb);
    HIPCHK(hipEventRecord(c->ek0, s), "event");
    HIPCHK(sidx_fa_bnd_count(dd, n, lnl, lgt, cnl, cgt, tcnt, toff, slot, tmp, &fb, s), "boundaries");
    if (nt)
      if (int rc = scan_total(c, toff, tcnt, nt, &K, res)) return rc;
    HIPCHK(sidx_scan_u64(nullptr, nullptr, K ? K : 1, nullptr, &tb, s), "scan size");
    if (int rc = c->d_sub.ensure(8 * (K + 1) + 48 * (K + 1) + tb + 4096, res)) return rc;
    u64 *Bw = c->d_sub.as<u64>();
    HIPCHK(sidx_fa_bnd_write(dd, n, cnl, cgt, tcnt, toff, slot, Bw, s), "boundary positions");
    B = Bw;
  } else if (!fasta) {
    const int brc = build_resident(c, dd, n, SHOCKIDX_LINE, SHOCKIDX_FMT_AUTO, s, &br);  // ReadBytes('\n')
    if (brc != SHOCKIDX_OK) return forward_error(res, br, brc < 0 ? brc : SHOCKIDX_EINTERNAL);
    res->kernel_ms += br.kernel_ms;
    K = br.count;
    B = c->d_rows;
    HIPCHK(sidx_scan_u64(nullptr, nullptr, K ? K : 1, nullptr, &tb, s), "scan size");
    if (int rc = c->d_sub.ensure(48 * (K + 1) + tb + 4096, res)) return rc;
    HIPCHK(hipEventRecord(c->ek0, s), "event");
  }
  Carver cv{c->d_sub};
  if (fasta) (void)cv.take<u64>(K + 1);  // the boundary positions
  u64 *small = cv.take<u64>(4);
  u64 *span = cv.take<u64>(2 * (K + 1));
  u64 *outlen = cv.take<u64>(K + 1);
  u64 *outoff = cv.take<u64>(K + 1);
  void *scan_tmp = cv.take<uint8_t>(tb);
  HIPCHK(hipMemsetAsync(small, 0xFF, 16, s), "memset");
  HIPCHK(hipMemsetAsync(small + 2, 0, 8, s), "memset");
  if (fasta) HIPCHK(sidx_fa_anon_spans(dd, n, B, bstride, K, span, outlen, small, s), "anonymize spans");
  else HIPCHK(sidx_sam_anon_spans(dd, n, B, K, span, outlen, small, small + 1, s), "anonymize spans");
  u64 st[2] = {~0ull, ~0ull};
  HIPCHK(hipMemcpyAsync(st, small, 16, hipMemcpyDeviceToHost, s), "status copy");
  HIPCHK(hipStreamSynchronize(s), "status sync");
  const u64 bad = st[0], eof = fasta ? ~0ull : st[1];
  const u64 Ke = bad < K && bad < eof ? bad : (eof < K ? eof : K);  // the items Read delivers
  const bool err = bad < K && bad < eof;
  u64 total = 0;
  if (int rc = scan_lengths(c, outlen, outoff, Ke, scan_tmp, &tb, &total, res)) return rc;
  res->size = total;
  res->count = fasta ? Ke : 0;
  if (size_only && !fasta) {  // SAM counts its lines as it writes them: the delivered ones (outlen != 0) here
    std::vector<u64> ol(Ke);
    if (Ke) HIPCHK(hipMemcpyAsync(ol.data(), outlen, 8 * Ke, hipMemcpyDeviceToHost, s), "length copy");
    HIPCHK(hipStreamSynchronize(s), "length sync");
    for (u64 v : ol) res->count += v != 0;
  }
  if (size_only) {
    res->total_ms = now_ms() - t0;
    return err ? set_msg(res, SHOCKIDX_EFORMAT, fasta ? "Invalid fasta entry" : "sam alignment fields less than 11")
               : SHOCKIDX_OK;
  }
  if (total > out_cap) return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
  if (fasta) HIPCHK(sidx_fa_anon_write(dd, n, span, outoff, Ke, d_out, s), "anonymize write");
  else HIPCHK(sidx_sam_anon_write(dd, span, outlen, outoff, Ke, d_out, small + 2, s), "anonymize write");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  if (!fasta) {
    u64 cnt = 0;
    if (int rc = d2h(c, &cnt, small + 2, res)) return rc;
    res->count = cnt;
  }
  HIPCHK(hipStreamSynchronize(s), "anonymize sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms += ms;
  res->total_ms = now_ms() - t0;
  if (!err) return SHOCKIDX_OK;
  return set_msg(res, SHOCKIDX_EFORMAT, fasta ? "Invalid fasta entry" : "sam alignment fields less than 11");
}

}  // namespace

namespace sidx_host {

int filter_kind(const char *filter) {  // filter.go:13-16
  if (!strcmp(filter, "fq2fa")) return 1;
  if (!strcmp(filter, "anonymize")) return 2;
  return 0;
}

// One section through its filter (res reset by the caller).  size_only: nothing is written and
// out_cap is not looked at -- the section's own status (OK or EFORMAT with Go's text) comes back
// with count / size = what a write would deliver (the sectioned stream sizes its output first).
int filter_section(shockidx_ctx *c, int kind, const uint8_t *dd, u64 n, void *d_out, u64 out_cap,
                   shockidx_subset_result *res, bool size_only) {
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  if (kind == 2) {  // anonymize reads through multi.Reader: DetermineFormat first (multi.go:43-62)
    int kfmt = 0;
    if (int rc = resolve_format(c, dd, n, SHOCKIDX_RECORD, SHOCKIDX_FMT_AUTO, s, &kfmt, res)) return rc;
    if (kfmt != SHOCKIDX_FMT_FASTQ) return anonymize_other(c, dd, n, kfmt, (uint8_t *)d_out, out_cap, res, t0, size_only);
  }
  // the record index (GetReadOffset) gives the record boundaries up to its first error; its tile
  // pass keeps every record's line ends for the spans
  shockidx_result br;
  reset_result(&br);
  c->want_spans = !getenv("SHOCKIDX_FILTER_RESCAN");
  const int brc = build_resident(c, dd, n, SHOCKIDX_RECORD, SHOCKIDX_FMT_FASTQ, s, &br);
  c->want_spans = false;
  if (brc < 0) return forward_error(res, br, brc);
  const u64 K = br.count;
  res->kernel_ms += br.kernel_ms;
  size_t scan_bytes = 0;
  HIPCHK(sidx_scan_u64(nullptr, nullptr, K ? K : 1, nullptr, &scan_bytes, s), "scan size");
  // the output blocks' first records: the output is at most the section + 11 bytes per record
  const u64 nwf = (n + 11 * K) / sidx_filter_block() + 4;
  const u64 need = 48 * (K + 8) + scan_bytes + 8 * nwf + 4096;
  if (int rc = c->d_sub.ensure(need, res)) return rc;
  Carver cv{c->d_sub};
  u64 *small = cv.take<u64>(8);
  u32 *spans = cv.take<u32>(6 * (K + 1));
  u64 *outlen = cv.take<u64>(K + 1);
  u64 *outoff = cv.take<u64>(K + 1);
  void *scan_tmp = cv.take<uint8_t>(scan_bytes);
  u64 *wfirst = cv.take<u64>(nwf);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(hipMemsetAsync(small, 0xFF, 8, s), "memset");
  if (c->last_spans && K) {  // the certified records' spans from the tile pass; k_fq_spans does the rest
    HIPCHK(hipMemsetAsync(outlen, 0, 8 * K, s), "memset");
    HIPCHK(sidx_launch_fq_spans_place(&c->last_p, spans, outlen, K, kind, s), "spans place");
  }
  HIPCHK(sidx_filter_spans(dd, n, c->d_rows, K, kind, spans, outlen, small, nullptr, s), "filter spans");
  u64 firstbad = ~0ull;
  if (int rc = d2h(c, &firstbad, small, res)) return rc;
  // Read()'s first failing record: one the index accepted but Read rejects (a blank-looking ID
  // or sequence line), else the index's own terminal record re-checked in Read's order
  u64 Ke = K;
  u32 code = ST_END;
  if (firstbad != ~0ull) {
    Ke = firstbad >> 4;
    code = (u32)(firstbad & 15);
  } else if (brc == SHOCKIDX_EFORMAT) {
    u64 last[2] = {0, 0};
    if (K) HIPCHK(hipMemcpyAsync(last, c->d_rows + 2 * (K - 1), 16, hipMemcpyDeviceToHost, s), "row copy");
    HIPCHK(sidx_filter_read_status(dd, n, K ? last[0] + last[1] : 0, (u32 *)(small + 1), s), "read status");
    u32 st = 0;
    if (int rc = d2h(c, &st, small + 1, res)) return rc;
    if (st == ST_OK || st == ST_END) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: filter terminal record");
    code = st;
  } else if (K) {  // the last record's quality line ends at EOF: Read returns it with io.EOF, dropped
    u64 last[2] = {0, 0};
    uint8_t lastb = '\n';
    HIPCHK(hipMemcpyAsync(last, c->d_rows + 2 * (K - 1), 16, hipMemcpyDeviceToHost, s), "row copy");
    if (n) HIPCHK(hipMemcpyAsync(&lastb, dd + n - 1, 1, hipMemcpyDeviceToHost, s), "byte copy");
    HIPCHK(hipStreamSynchronize(s), "sync");
    if (last[0] + last[1] == n && lastb != '\n') Ke = K - 1;
  }
  u64 total = 0;
  if (int rc = scan_lengths(c, outlen, outoff, Ke, scan_tmp, &scan_bytes, &total, res)) return rc;
  res->count = Ke;
  res->size = total;
  if (!size_only) {
    if (total > out_cap) return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
    if (total / sidx_filter_block() + 1 > nwf) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: filter plan size");
    HIPCHK(sidx_filter_write(dd, n, c->d_rows, spans, outlen, outoff, Ke, total, kind, wfirst, (uint8_t *)d_out, nullptr,
                             s),
           "filter write");
  }
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipStreamSynchronize(s), "filter sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms += ms;
  res->total_ms = now_ms() - t0;
  if (code == ST_END) return SHOCKIDX_OK;
  const char *m = status_message(code);
  return set_msg(res, SHOCKIDX_EFORMAT, m ? m : "internal error: filter status");
}

}  // namespace sidx_host

// ---- the filters in slabs ----------------------------------------------------------------------
namespace {

// the slab step's control words live where the chunkrecord slab step's do: a context runs one slab
// step at a time, and neither keeps anything there between calls
u64 *filt_st(shockidx_ctx *c) { return (u64 *)(c->d_small + SMALL_CHUNK); }
static_assert(SMALL_CHUNK + FS_WORDS * sizeof(u64) <= SMALL_BYTES, "small layout");

// eight control words from `src`, waited for
int read_words(shockidx_ctx *c, hipStream_t s, const u64 *src, u64 h[8], Err res) {
  HIPCHK(hipMemcpyAsync(c->h_det, src, 8 * sizeof(u64), hipMemcpyDeviceToHost, s), "filter slab copy");
  HIPCHK(hipStreamSynchronize(s), "filter slab sync");
  memcpy(h, c->h_det, 8 * sizeof(u64));
  return 0;
}

// an ended carry with nothing delivered (the first slab of anonymize over a section of no format)
int end_carry(shockidx_ctx *c, int kind, FiltCarry *carry, hipStream_t s, Err res) {
  u64 h[FS_WORDS] = {0};
  h[FS_KIND] = (u64)kind;
  h[FS_ENDED] = 1;
  HIPCHK(hipMemcpyAsync(filt_st(c), h, sizeof h, hipMemcpyHostToDevice, s), "filter slab copy");
  HIPCHK(sidx_filt_slab_commit(carry, filt_st(c), 1, s), "filter carry launch");
  HIPCHK(hipStreamSynchronize(s), "filter slab sync");
  return 0;
}

}  // namespace

namespace sidx_host {

FiltWalkDev filter_walk_dev(shockidx_ctx *c, u64 len) {
  size_t sb = 0;
  (void)sidx_scan_u64(nullptr, nullptr, filtwalk_rows_cap(len), nullptr, &sb, c->stream);
  return FiltWalkDev{(sizeof(FiltCarry) + 255) & ~255ull, sb, sidx_filter_block(), c->tiles_grid};
}

// One slab over the window [wlo, whi) at win (d_data - front), owned up to own_end: three host
// stops of its own (the carry and the view's end; the delivered records, their bytes and Read's
// status; the written output) and the record index's.  Returns like shockidx_filter_slab_device.
int filter_slab_run(shockidx_ctx *c, int kind, const uint8_t *win, u64 wlo, u64 whi, u64 own_end, bool first, bool last,
                    u64 sec_size, FiltCarry *carry, uint8_t *d_out, u64 out_cap, u64 *next_pos,
                    shockidx_subset_result *res) {
  hipStream_t s = c->stream;
  u64 *st = filt_st(c);
  u64 h[8];
  HIPCHK(sidx_filt_slab_begin(win, wlo, whi, own_end, first, last, kind, carry, st, s), "filter slab launch");
  if (int rc = read_words(c, s, st, h, res)) return rc;
  if (next_pos) *next_pos = h[FS_POS];
  if (h[FS_STATUS] == FSS_ENDED) return set_msg(res, SHOCKIDX_EINVAL, "filter slab: the carry's stream has ended");
  if (h[FS_STATUS] == FSS_KIND) return set_msg(res, SHOCKIDX_EINVAL, "filter slab: the carry belongs to the other filter");
  if (h[FS_STATUS] != FSS_OK)
    return set_msg(res, SHOCKIDX_EINVAL, "filter slab: the carried position lies outside the slab's window and owned bytes");
  const u64 pos = h[FS_POS], vn = h[FS_VEND] - pos, cbase = h[FS_COUNT];
  // the view at a 16-byte-aligned address (the carried position is wherever the last record ended)
  if (int rc = c->d_fview.ensure(vn + FILTWALK_PAD, res)) return rc;
  const uint8_t *view = c->d_fview;
  if (vn) HIPCHK(hipMemcpyAsync(c->d_fview, win + (pos - wlo), vn, hipMemcpyDeviceToDevice, s), "view copy");
  shockidx_result br;
  reset_result(&br);
  const int brc = build_resident(c, view, vn, SHOCKIDX_RECORD, SHOCKIDX_FMT_FASTQ, s, &br);
  if (brc < 0) return forward_error(res, br, brc);
  const u64 K = br.count;
  res->kernel_ms += br.kernel_ms;
  size_t scan_bytes = 0;
  HIPCHK(sidx_scan_u64(nullptr, nullptr, K ? K : 1, nullptr, &scan_bytes, s), "scan size");
  const u64 bound = filtwalk_out_bound(vn, K, cbase + K);
  if (int rc = c->d_sub.ensure(filtwalk_ws_bytes(K, bound, scan_bytes, sidx_filter_block()), res)) return rc;
  Carver cv{c->d_sub};
  (void)cv.take<u64>(8);
  u32 *spans = cv.take<u32>(6 * (K + 1));
  u64 *outlen = cv.take<u64>(K + 1);
  u64 *outoff = cv.take<u64>(K + 1);
  void *scan_tmp = cv.take<uint8_t>(scan_bytes);
  const u64 nwf = bound / sidx_filter_block() + 4;
  u64 *wfirst = cv.take<u64>(nwf);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(hipMemsetAsync(st + FS_KE, 0, 7 * sizeof(u64), s), "memset");
  HIPCHK(hipMemsetAsync(st + FS_FIRSTBAD, 0xFF, sizeof(u64), s), "memset");
  if (K) {
    HIPCHK(hipMemsetAsync(outlen, 0, 8 * K, s), "memset");  // (no span carries the tile pass's mark)
    HIPCHK(sidx_filter_spans_base(view, vn, c->d_rows, K, kind, spans, outlen, st + FS_FIRSTBAD, st + FS_COUNT, s), "filter spans");
    HIPCHK(sidx_scan_u64(outlen, outoff, K, scan_tmp, &scan_bytes, s), "scan");
  }
  HIPCHK(sidx_filt_slab_settle(view, vn, c->d_rows, K, brc == SHOCKIDX_EFORMAT, last && own_end == whi ? ~0ull : own_end - pos, last, outlen,
                               outoff, sec_size, st, s),
         "filter settle launch");
  if (int rc = read_words(c, s, st + FS_KE, h, res)) return rc;
  const u64 ke = h[FS_KE - FS_KE], total = h[FS_TOTAL - FS_KE], newpos = h[FS_NEWPOS - FS_KE];
  const u32 code = (u32)h[FS_CODE - FS_KE];
  if (code == FS_CODE_INTERNAL) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: filter terminal record");
  res->count = ke;
  res->size = total;
  if (total > out_cap) return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
  if (total / sidx_filter_block() + 1 > nwf) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: filter plan size");
  HIPCHK(sidx_filter_write_base(view, vn, c->d_rows, spans, outlen, outoff, ke, total, kind, wfirst, d_out, st + FS_COUNT, s),
         "filter write");
  HIPCHK(sidx_filt_slab_commit(carry, st, first, s), "filter carry launch");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipStreamSynchronize(s), "filter sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms += ms;
  if (next_pos) *next_pos = newpos;
  if (code == ST_END) return SHOCKIDX_OK;
  const char *m = status_message(code);
  return set_msg(res, SHOCKIDX_EFORMAT, m ? m : "internal error: filter status");
}

}  // namespace sidx_host

// ---- Download filters on device: fq2fa / anonymize (node/filter/) --------------------------
extern "C" {

uint64_t shockidx_filter_carry_bytes(void) { return sizeof(FiltCarry); }

// One slab of a section through fq2fa / anonymize (the reader of fastq.go:50-132 with its position
// and the filter's counter carried from slab to slab).
int shockidx_filter_slab_device(shockidx_ctx *c, const char *filter, const shockidx_slab *slab, uint64_t sec_size,
                                void *d_carry, void *d_out, uint64_t out_cap, uint64_t *next_pos,
                                shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !filter || !slab || !d_carry || ((uintptr_t)d_carry & 7) || (!d_out && out_cap))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const int kind = filter_kind(filter);
  if (!kind) return set_msg(res, SHOCKIDX_EINVAL, "unknown filter");
  const shockidx_slab &b = *slab;
  const bool first = b.is_first != 0, last = b.end <= sec_size && b.base == sec_size - b.end;
  if (b.front > b.base || b.base > sec_size || b.end > sec_size - b.base || b.n > b.end || (b.front + b.end && !b.d_data) ||
      ((uintptr_t)b.d_data & 15) || (b.is_last != 0) != last)
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const uint8_t *win = (const uint8_t *)b.d_data - b.front;
  const u64 wlo = b.base - b.front, whi = b.base + b.end;
  if (first && kind == 2) {  // anonymize reads through multi.Reader: DetermineFormat first (multi.go:43-62)
    const u64 need = sec_size < FILTWALK_DETECT ? sec_size : FILTWALK_DETECT;
    if (wlo != 0 || whi < need || ((uintptr_t)win & 15))
      return set_msg(res, SHOCKIDX_EINVAL, "filter slab: format detection needs the section's first 32 KiB in the first slab");
    int kfmt = 0;
    if (int rc = resolve_format(c, win, whi, SHOCKIDX_RECORD, SHOCKIDX_FMT_AUTO, s, &kfmt, res)) {
      if (rc == SHOCKIDX_EFORMAT) {  // no format: the stream ends with Go's error, nothing delivered
        if (int rc2 = end_carry(c, kind, (FiltCarry *)d_carry, s, res)) return rc2;
        if (next_pos) *next_pos = 0;
      }
      return rc;
    }
    if (kfmt != SHOCKIDX_FMT_FASTQ)
      return set_msg(res, SHOCKIDX_EINVAL, kfmt == SHOCKIDX_FMT_FASTA
                                               ? "filter slab: the section detects as FASTA (only FASTQ sections are filtered in slabs)"
                                               : "filter slab: the section detects as SAM (only FASTQ sections are filtered in slabs)");
  }
  const int rc = filter_slab_run(c, kind, win, wlo, whi, b.base + b.n, first, last, sec_size, (FiltCarry *)d_carry,
                                 (uint8_t *)d_out, out_cap, (u64 *)next_pos, res);
  res->total_ms = now_ms() - t0;
  return rc;
}

int shockidx_filter_fd_walk(shockidx_ctx *c, const char *filter, int fd, uint64_t off, uint64_t n, int out_fd,
                            uint64_t slab_bytes, uint64_t halo_bytes, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !filter || fd < 0 || out_fd < 0 || (slab_bytes && slab_bytes < FILTWALK_DETECT))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const int kind = filter_kind(filter);
  if (!kind) return set_msg(res, SHOCKIDX_EINVAL, "unknown filter");
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  return filter_fd_walk(c, kind, filter, fd, off, n, out_fd, slab_bytes, halo_bytes, res);
}

int shockidx_filter_fd(shockidx_ctx *c, const char *filter, int fd, uint64_t off, uint64_t n, int out_fd,
                       shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !filter || fd < 0 || out_fd < 0) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const int kind = filter_kind(filter);
  if (!kind) return set_msg(res, SHOCKIDX_EINVAL, "unknown filter");
  TrimGuard trim{c};
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  return filter_fd_any(c, kind, filter, fd, off, n, out_fd, res);
}

int shockidx_filter_last_stats(const shockidx_ctx *c, shockidx_filter_stats *out) {
  if (!c || !out) return SHOCKIDX_EINVAL;
  *out = c->filter_stats;
  return SHOCKIDX_OK;
}

int shockidx_filter_device(shockidx_ctx *c, const char *filter, const void *d_data, uint64_t n, void *d_out,
                           uint64_t out_cap, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !filter || (!d_data && n) || ((uintptr_t)d_data & 15) || (!d_out && out_cap))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const int kind = filter_kind(filter);
  if (!kind) return set_msg(res, SHOCKIDX_EINVAL, "unknown filter");
  return filter_section(c, kind, (const uint8_t *)d_data, n, d_out, out_cap, res, false);
}

}  // extern "C"
