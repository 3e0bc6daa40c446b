// sidx_subset_api.cpp -- subset nodes (subset.go) and the index read path (Idx.Part / Idx.Range,
// index/index.go) of the C ABI, over the kernels of sidx_subset.hip.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_subset.hpp"
#include "sidx_launch.hpp"
#include "sidx_host.hpp"
#include "sidx_plan_host.hpp"

using namespace sidx;
using namespace sidx_host;
using namespace sidx_plan;  // the part strings and Go's error texts

// ---- Subset nodes ------------------------------------------------------------------------
namespace {

// strconv.Quote (strconv/quote.go appendQuotedWith / appendEscapedRune) for the Atoi error
// text; unicode.IsPrint exact for ASCII and Latin-1, approximated above.
u32 go_decode_rune(const uint8_t *s, size_t n, size_t *w) {
  const u32 c0 = s[0];
  if (c0 < 0x80) { *w = 1; return c0; }
  u32 sz = 0, lo = 0x80, hi = 0xBF;
  if (c0 >= 0xC2 && c0 <= 0xDF) sz = 2;
  else if (c0 == 0xE0) { sz = 3; lo = 0xA0; }
  else if ((c0 >= 0xE1 && c0 <= 0xEC) || c0 == 0xEE || c0 == 0xEF) sz = 3;
  else if (c0 == 0xED) { sz = 3; hi = 0x9F; }
  else if (c0 == 0xF0) { sz = 4; lo = 0x90; }
  else if (c0 >= 0xF1 && c0 <= 0xF3) sz = 4;
  else if (c0 == 0xF4) { sz = 4; hi = 0x8F; }
  if (!sz || n < sz || s[1] < lo || s[1] > hi) { *w = 1; return 0xFFFD; }
  for (u32 i = 2; i < sz; ++i)
    if (s[i] < 0x80 || s[i] > 0xBF) { *w = 1; return 0xFFFD; }
  *w = sz;
  if (sz == 2) return ((c0 & 0x1F) << 6) | (s[1] & 0x3F);
  if (sz == 3) return ((c0 & 0x0F) << 12) | ((u32)(s[1] & 0x3F) << 6) | (s[2] & 0x3F);
  return ((c0 & 0x07) << 18) | ((u32)(s[1] & 0x3F) << 12) | ((u32)(s[2] & 0x3F) << 6) | (s[3] & 0x3F);
}
bool go_is_print(u32 r) {
  if (r < 0x80) return r >= 0x20 && r < 0x7F;
  if (r <= 0xA0 || r == 0xAD) return false;
  if (r < 0x100) return true;
  return !(r == 0x1680 || (r >= 0x2000 && r <= 0x200F) || (r >= 0x2028 && r <= 0x202F) ||
           (r >= 0x205F && r <= 0x206F) || r == 0x3000 || r == 0xFEFF || (r >= 0xFFF9 && r <= 0xFFFB) ||
           (r >= 0xD800 && r <= 0xDFFF) || r > 0x10FFFF);
}
std::string go_quote(const uint8_t *s, size_t n) {
  static const char hx[] = "0123456789abcdef";
  std::string q = "\"";
  for (size_t i = 0; i < n;) {
    size_t w;
    const u32 r = go_decode_rune(s + i, n - i, &w);
    if (w == 1 && r == 0xFFFD) {
      q += "\\x"; q += hx[s[i] >> 4]; q += hx[s[i] & 15];
    } else if (r == '"' || r == '\\') {
      q += '\\'; q += (char)r;
    } else if (go_is_print(r)) {
      q.append((const char *)s + i, w);
    } else if (r == '\a') q += "\\a";
    else if (r == '\b') q += "\\b";
    else if (r == '\f') q += "\\f";
    else if (r == '\n') q += "\\n";
    else if (r == '\r') q += "\\r";
    else if (r == '\t') q += "\\t";
    else if (r == '\v') q += "\\v";
    else if (r < ' ' || r == 0x7F) { q += "\\x"; q += hx[r >> 4]; q += hx[r & 15]; }
    else if (r < 0x10000) { q += "\\u"; for (int sh = 12; sh >= 0; sh -= 4) q += hx[(r >> sh) & 15]; }
    else { q += "\\U"; for (int sh = 28; sh >= 0; sh -= 4) q += hx[(r >> sh) & 15]; }
    i += w;
  }
  q += '"';
  return q;
}

// Go's error text for a failing id (subset.go:203-223): txt, the first k bytes of its line, for Atoi's two
std::string subset_error_text(u32 code, i64 v, i64 prev, const uint8_t *txt, u64 k) {
  if (code == SUB_SYNTAX || code == SUB_RANGE)
    return "strconv.Atoi: parsing " + go_quote(txt, k) + ": " + (code == SUB_SYNTAX ? "invalid syntax" : "value out of range");
  char buf[256];
  if (code == SUB_SORT)
    snprintf(buf, sizeof buf,
             "Subset indices must be numerically sorted and non-redundant, found value %lld after value %lld",
             (long long)v, (long long)prev);
  else if (code == SUB_EXIST)
    snprintf(buf, sizeof buf, "Subset index: %lld does not exist in parent index file.", (long long)v);
  else
    snprintf(buf, sizeof buf, "Subset index could not read parent index file for part: %lld", (long long)v);
  return buf;
}

// CreateSubsetNodeIndexes (subset.go:133-303) on the device, and optionally the subset node's
// bytes (single.go:500-517): the id lines (the line index kernel), then every count -- the
// non-blank ids, the first failing one, the accepted ids, the runs, oSize, the gathered bytes --
// stays on the device (SubCtl words) and the kernels read it there, so the host waits twice:
// for the id line count and once at the end.  d_data == nullptr: no gather.
int subset_build(shockidx_ctx *c, const void *d_ids, uint64_t ids_len, const void *d_parent, uint64_t parent_count,
                 int64_t ilength, void *d_rows, uint64_t rows_cap, void *d_runs, uint64_t runs_cap, const void *d_data,
                 uint64_t data_len, void *d_out, uint64_t out_cap, shockidx_subset_result *res) {
  reset_result(res);
  if (!c || (!d_ids && ids_len) || ((uintptr_t)d_ids & 15) || (!d_parent && parent_count) ||
      (d_data && (((uintptr_t)d_data & 15) || ((uintptr_t)d_out & 15) || !d_runs)))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  // 1. lines of the id text (subset.go:189-199, ReadLine = ReadBytes('\n')): the position of
  // every '\n' (sidx_id_lines) into the context's row workspace, then their count to the host;
  // the bytes after the last '\n' are dropped like ReadLine's EOF line
  const u64 nb = (ids_len + 1023) / 1024;
  size_t ltmp = 0;
  HIPCHK(sidx_id_lines(nullptr, ids_len, nullptr, nullptr, nullptr, nullptr, &ltmp, s), "scan size");
  const u64 ends_bytes = (8 * (ids_len + 2) + 255) / 256 * 256;
  const u64 lbytes = ends_bytes + (4 * nb + 255) / 256 * 256 + (8 * nb + 255) / 256 * 256 + (ltmp + 255) / 256 * 256 + 256;
  if (int rc = c->d_rows.ensure((lbytes + 15) / 16, res)) return rc;
  u64 *ends = c->d_rows;
  u64 m = 0;
  {
    Carver lc{c->d_rows.as<uint8_t>() + ends_bytes};
    u32 *cnt = lc.take<u32>(nb);
    u64 *base = lc.take<u64>(nb);
    void *tmp = lc.take<uint8_t>(ltmp);
    HIPCHK(hipEventRecord(c->ek0, s), "event");
    HIPCHK(sidx_id_lines((const uint8_t *)d_ids, ids_len, cnt, base, ends, tmp, &ltmp, s), "id lines");
    HIPCHK(hipEventRecord(c->ek1, s), "event");
    u64 b_last = 0;
    u32 c_last = 0;
    if (nb) {
      HIPCHK(hipMemcpyAsync(&b_last, base + nb - 1, 8, hipMemcpyDeviceToHost, s), "line count copy");
      HIPCHK(hipMemcpyAsync(&c_last, cnt + nb - 1, 4, hipMemcpyDeviceToHost, s), "line count copy");
    }
    HIPCHK(hipStreamSynchronize(s), "line count sync");
    m = b_last + c_last;
    float lms = 0.f;
    (void)hipEventElapsedTime(&lms, c->ek0, c->ek1);
    res->kernel_ms += lms;
  }
  // 2. workspace (every count is bounded by m; the gather's runs by min(m, runs_cap))
  const bool gather = d_data != nullptr;
  const u64 gb = gather ? (m < runs_cap ? m : runs_cap) : 0;
  size_t scan_bytes = 0, gscan = 0;
  HIPCHK(sidx_scan_flags(nullptr, nullptr, m ? m : 1, nullptr, &scan_bytes, s), "scan size");
  if (gather)
    HIPCHK(sidx_gather(nullptr, 0, nullptr, gb, nullptr, nullptr, nullptr, nullptr, &gscan, nullptr, nullptr, 0, nullptr,
                       nullptr, s),
           "scan size");
  const u64 gblocks = gather ? (out_cap < data_len ? out_cap : data_len) / sidx::GATHER_BLOCK + 2 : 0;
  const u64 need = 8 * SC_ALLWORDS + 64 * (m + 8) + scan_bytes + 16 * (gb + 8) + gscan + 8 * gblocks + 4096;
  if (int rc = c->d_sub.ensure(need, res)) return rc;
  Carver cv{c->d_sub};
  u64 *ctl = cv.take<u64>(SC_ALLWORDS);
  u32 *keep = cv.take<u32>(m + 1);
  i64 *val = cv.take<i64>(m + 1);
  u32 *st = cv.take<u32>(m + 1);
  u64 *rank = cv.take<u64>(m + 1);
  i64 *cval = cv.take<i64>(m + 1);
  u32 *cst = cv.take<u32>(m + 1);
  u64 *cline = cv.take<u64>(m + 1);
  void *scan_tmp = cv.take<uint8_t>(scan_bytes);
  u64 *lens = cv.take<u64>(gb + 1), *outoff = cv.take<u64>(gb + 1);
  void *gtmp = cv.take<uint8_t>(gscan);
  u64 *wfirst = cv.take<u64>(gblocks);
  u32 *startf = keep;  // reused after compaction
  u64 *runid = rank;
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(sidx_subset_init(ctl, 0, s), "init");
  if (m) {
    HIPCHK(sidx_subset_parse((const uint8_t *)d_ids, ends, m, keep, val, st, s), "parse");
    HIPCHK(sidx_scan_flags(keep, rank, m, scan_tmp, &scan_bytes, s), "scan");
    HIPCHK(sidx_subset_compact(keep, rank, val, st, m, cval, cst, cline, ctl, s), "compact");
  }
  // 3. per-id checks, row gather, run starts, Ke; 4. runs and oSize
  HIPCHK(sidx_subset_check(cval, cst, m, ctl, (const u64 *)d_parent, parent_count, ilength, (u64 *)d_rows, rows_cap,
                           startf, s),
         "check");
  if (m) HIPCHK(sidx_scan_flags(startf, runid, m, scan_tmp, &scan_bytes, s), "scan");
  HIPCHK(sidx_subset_runs((const u64 *)d_rows, startf, runid, m, ctl, (u64 *)d_runs, rows_cap, runs_cap, s), "runs");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  // 5. the node's bytes, when asked for (skipped on the device after an error or a short capacity)
  if (gather)
    HIPCHK(sidx_gather((const uint8_t *)d_data, data_len, (const u64 *)d_runs, gb, ctl, lens, outoff, gtmp, &gscan,
                       wfirst, (uint8_t *)d_out, out_cap, c->ev0, c->ev1, s),
           "gather");
  u64 w[SC_ALLWORDS];
  HIPCHK(hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
  HIPCHK(hipStreamSynchronize(s), "subset sync");
  for (int i = 0; i < SC_SLOTS; ++i) w[SC_SIZE] += w[SC_NWORDS + i];  // oSize (k_sub_runs' slots)
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms += ms;
  if (gather) {
    float gms = 0.f;
    (void)hipEventElapsedTime(&gms, c->ev0, c->ev1);
    res->gather_ms = gms;
  }
  const u64 firstbad = w[SC_FIRSTBAD], Ke = w[SC_KE], nstart = w[SC_NSTART], size = w[SC_SIZE];
  const bool bad = firstbad != ~0ull;
  res->total_ms = now_ms() - t0;
  if (w[SC_FLAGS] & 1) {
    res->count = Ke;
    return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  }
  if (w[SC_FLAGS] & 2) {
    res->count = Ke;
    res->runs = nstart;
    return set_msg(res, SHOCKIDX_ESPACE, "run capacity too small");
  }
  res->count = Ke;
  res->size = size;
  // coCount: runs flushed by subset.go:245-261, plus the final one when oSize != 0 (:285-291);
  // at an error the open run was never flushed
  res->runs = bad ? (nstart ? nstart - 1 : 0) : (size ? nstart : (nstart ? nstart - 1 : 0));
  if (gather && !bad) {
    if (w[SC_FLAGS] & 8) return set_msg(res, SHOCKIDX_EINVAL, "runs exceed the data");
    if (w[SC_FLAGS] & 4) return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
  }
  if (!bad) return SHOCKIDX_OK;
  // Go's error text for the first failing id
  const u64 r = firstbad >> 3;
  const u32 code = (u32)(firstbad & 7);
  i64 v = 0, prev = 0;
  if (int rc = d2h(c, &v, cval + r, res)) return rc;
  if (r) {
    if (int rc = d2h(c, &prev, cval + r - 1, res)) return rc;
  }
  uint8_t txt[200];
  u64 k = 0;
  if (code == SUB_SYNTAX || code == SUB_RANGE) {
    u64 li = 0, ln[2];
    if (int rc = d2h(c, &li, cline + r, res)) return rc;
    u64 e2[2] = {~0ull, 0};  // ends[li - 1], ends[li]: line li is [ends[li - 1] + 1, ends[li]]
    HIPCHK(hipMemcpyAsync(li ? e2 : e2 + 1, c->d_rows + (li ? li - 1 : 0), li ? 16 : 8, hipMemcpyDeviceToHost, s),
           "line copy");
    HIPCHK(hipStreamSynchronize(s), "sync");
    ln[0] = e2[0] + 1;  // (li == 0: ~0 + 1 = 0)
    ln[1] = e2[1] + 1 - ln[0];
    k = ln[1] - 1 < 200 ? ln[1] - 1 : 200;  // enough for a 255-byte message
    if (k) {
      HIPCHK(hipMemcpyAsync(txt, (const uint8_t *)d_ids + ln[0], k, hipMemcpyDeviceToHost, s), "text copy");
      HIPCHK(hipStreamSynchronize(s), "sync");
    }
  }
  return set_msg(res, SHOCKIDX_EFORMAT, subset_error_text(code, v, prev, txt, k));
}

}  // namespace

extern "C" {

int shockidx_subset_index(shockidx_ctx *c, const void *d_ids, uint64_t ids_len, const void *d_parent,
                          uint64_t parent_count, int64_t ilength, void *d_rows, uint64_t rows_cap, void *d_runs,
                          uint64_t runs_cap, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  return subset_build(c, d_ids, ids_len, d_parent, parent_count, ilength, d_rows, rows_cap, d_runs, runs_cap, nullptr,
                      0, nullptr, 0, res ? res : &tmp);
}

int shockidx_subset_node(shockidx_ctx *c, const void *d_ids, uint64_t ids_len, const void *d_parent,
                         uint64_t parent_count, int64_t ilength, void *d_rows, uint64_t rows_cap, void *d_runs,
                         uint64_t runs_cap, const void *d_data, uint64_t data_len, void *d_out, uint64_t out_cap,
                         shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!d_data) {
    if (!res) res = &tmp;
    reset_result(res);
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  }
  return subset_build(c, d_ids, ids_len, d_parent, parent_count, ilength, d_rows, rows_cap, d_runs, runs_cap, d_data,
                      data_len, d_out, out_cap, res ? res : &tmp);
}

int shockidx_subset_gather(shockidx_ctx *c, const void *d_data, uint64_t data_len, const void *d_runs, uint64_t nruns,
                           void *d_out, uint64_t out_cap, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || (!d_runs && nruns) || ((uintptr_t)d_data & 15) || ((uintptr_t)d_out & 15))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  res->runs = nruns;
  if (!nruns) return SHOCKIDX_OK;
  size_t scan_bytes = 0;
  HIPCHK(sidx_gather(nullptr, 0, nullptr, nruns, nullptr, nullptr, nullptr, nullptr, &scan_bytes, nullptr, nullptr, 0,
                     nullptr, nullptr, s),
         "scan size");
  // runs are disjoint pieces of the parent file, so the output is at most data_len bytes
  const u64 max_blocks = (out_cap < data_len ? out_cap : data_len) / sidx::GATHER_BLOCK + 2;
  const u64 need = 8 * SC_ALLWORDS + 16 * (nruns + 16) + scan_bytes + 8 * max_blocks + 4096;
  if (int rc = c->d_sub.ensure(need, res)) return rc;
  Carver cv{c->d_sub};
  u64 *ctl = cv.take<u64>(SC_ALLWORDS);
  u64 *lens = cv.take<u64>(nruns);
  u64 *outoff = cv.take<u64>(nruns);
  void *scan_tmp = cv.take<uint8_t>(scan_bytes);
  u64 *wfirst = cv.take<u64>(max_blocks);
  HIPCHK(sidx_subset_init(ctl, nruns, s), "init");
  HIPCHK(sidx_gather((const uint8_t *)d_data, data_len, (const u64 *)d_runs, nruns, ctl, lens, outoff, scan_tmp,
                     &scan_bytes, wfirst, (uint8_t *)d_out, out_cap, c->ek0, c->ek1, s),
         "gather");
  u64 w[SC_NWORDS];
  HIPCHK(hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
  HIPCHK(hipStreamSynchronize(s), "gather sync");
  res->size = w[SC_TOTAL];
  res->total_ms = now_ms() - t0;
  if (w[SC_FLAGS] & 8) return set_msg(res, SHOCKIDX_EINVAL, "runs exceed the data");
  if (w[SC_FLAGS] & 4) return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms = ms;
  return SHOCKIDX_OK;
}

int shockidx_create_subset_index(shockidx_ctx *c, const void *d_ids, uint64_t ids_len, const void *d_parent,
                                 uint64_t parent_count, int64_t ilength, void *d_rows, uint64_t rows_cap,
                                 shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  // subset.go:36-128: the same per-id checks and rows as CreateSubsetNodeIndexes, no
  // compressed index; every error returns (-1, -1, err)
  const int rc = shockidx_subset_index(c, d_ids, ids_len, d_parent, parent_count, ilength, d_rows, rows_cap, nullptr,
                                       0, res);
  res->runs = 0;
  if (rc == SHOCKIDX_EFORMAT) res->count = res->size = ~0ull;
  return rc;
}

}  // extern "C"

// ---- the subset builders one slab of the id text at a time (subset.go:186-291) ----------------
namespace sidx_host {

namespace {
u64 up256(u64 x) { return (x + 255) / 256 * 256; }
// c->d_sends: the ends (a '\n' per byte at worst), the 1 KiB blocks' counts and bases, the scan's temp
u64 subs_ends_bytes(u64 end, u64 ltmp) {
  const u64 nb = (end + 1023) / 1024;
  return up256(8 * (end + 2)) + up256(4 * nb) + up256(8 * nb) + up256(ltmp) + 256;
}
// c->d_sub: the control words and the per-line arrays for m lines
u64 subs_line_bytes(u64 m, u64 scan_bytes) { return up256(8 * SL_WORDS) + 7 * up256(8 * (m + 1)) + up256(scan_bytes) + 256; }
}  // namespace

void subset_slab_ws_parts(u64 end, u64 *ends_bytes, u64 *line_bytes) {
  size_t ltmp = 0, sb = 0;
  (void)sidx_id_lines(nullptr, end, nullptr, nullptr, nullptr, nullptr, &ltmp, nullptr);
  (void)sidx_scan_flags(nullptr, nullptr, end ? end : 1, nullptr, &sb, nullptr);  // (a line per byte at worst)
  *ends_bytes = subs_ends_bytes(end, ltmp);
  *line_bytes = subs_line_bytes(end, sb);
}
u64 subset_slab_ws_bytes(u64 end) {
  u64 a = 0, b = 0;
  subset_slab_ws_parts(end, &a, &b);
  return a + b;
}

u64 subset_whole_bytes(u64 ids_size, u64 parent_bytes) {
  // a bound: the two files, subset_build's ends (8 bytes per text byte), its per-line workspace (64
  // bytes a line, a line per byte when they are all blank) and both tables (a row per two bytes);
  // an eighth on top for DevBuf::ensure's growth
  const u64 b = ids_size + parent_bytes + 8 * (ids_size + 2) + 64 * (ids_size + 8) + 32 * (ids_size / 2 + 4096) +
                (1ull << 20);
  return b + b / 8;
}

}  // namespace sidx_host

extern "C" {

uint64_t shockidx_subset_carry_bytes(void) { return sizeof(SubCarry); }

// One slab of CreateSubsetNodeIndexes / CreateSubsetIndex (subset.go:186-291 with the loop's state,
// :161-176, in the device carry).  The host waits three times: for the window's line count, for the
// plan (where the call stops, what it writes) and for the commit.
int shockidx_subset_slab_device(shockidx_ctx *c, const shockidx_slab *slab, uint64_t ids_size, const void *d_parent,
                                uint64_t prow0, uint64_t prows, uint64_t parent_count, int64_t ilength, int want_runs,
                                void *d_carry, void *d_rows, uint64_t rows_cap, void *d_runs, uint64_t runs_cap,
                                shockidx_subset_slab_result *res) {
  shockidx_subset_slab_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !slab || !d_carry || (!d_rows && rows_cap) || (!d_runs && runs_cap) || (!d_parent && prows))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const shockidx_slab &b = *slab;
  const bool first = b.base == 0, last = b.base + b.n == ids_size;
  if (b.end < b.n || b.base > ids_size || b.end > ids_size - b.base || (!b.n && ids_size) ||
      (b.n && (!b.d_data || ((uintptr_t)b.d_data & 15))) || (b.is_first != 0) != first || (b.is_last != 0) != last ||
      b.front < (b.base < 16 ? b.base : 16) || b.front > b.base || ((uintptr_t)d_carry & 7) ||
      ((uintptr_t)d_parent & 15) || ((uintptr_t)d_rows & 15) || ((uintptr_t)d_runs & 15) ||
      prow0 > parent_count || prows > parent_count - prow0)
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const u64 end = b.end, nb = (end + 1023) / 1024;
  size_t ltmp = 0;
  HIPCHK(sidx_id_lines(nullptr, end, nullptr, nullptr, nullptr, nullptr, &ltmp, s), "scan size");
  if (int rc = c->d_sends.ensure(subs_ends_bytes(end, ltmp), res)) return rc;
  Carver lc{c->d_sends};
  u64 *ends = lc.take<u64>(end + 2);
  u32 *cnt = lc.take<u32>(nb);
  u64 *lbase = lc.take<u64>(nb);
  void *ltmp_p = lc.take<uint8_t>(ltmp);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  u64 m = 0;
  if (nb) {
    HIPCHK(sidx_id_lines((const uint8_t *)b.d_data, end, cnt, lbase, ends, ltmp_p, &ltmp, s), "id lines");
    u64 b_last = 0;
    u32 c_last = 0;
    HIPCHK(hipMemcpyAsync(&b_last, lbase + nb - 1, 8, hipMemcpyDeviceToHost, s), "line count copy");
    HIPCHK(hipMemcpyAsync(&c_last, cnt + nb - 1, 4, hipMemcpyDeviceToHost, s), "line count copy");
    HIPCHK(hipStreamSynchronize(s), "line count sync");
    m = b_last + c_last;
  }
  size_t scan_bytes = 0;
  HIPCHK(sidx_scan_flags(nullptr, nullptr, m ? m : 1, nullptr, &scan_bytes, s), "scan size");
  if (int rc = c->d_sub.ensure(subs_line_bytes(m, scan_bytes), res)) return rc;
  Carver cv{c->d_sub};
  SubSlabArgs a;
  memset(&a, 0, sizeof a);
  a.text = (const uint8_t *)b.d_data;
  a.n = b.n; a.end = end; a.front = b.front; a.base = b.base; a.ids_size = ids_size;
  a.is_first = first; a.is_last = last; a.want_runs = want_runs != 0;
  a.parent = (const u64 *)d_parent; a.prow0 = prow0; a.prows = prows; a.parent_count = parent_count;
  a.ilength = ilength;
  a.carry = (SubCarry *)d_carry;
  a.rows = (u64 *)d_rows; a.rows_cap = rows_cap; a.runs = (u64 *)d_runs; a.runs_cap = runs_cap;
  a.m = m;
  a.ends = ends;
  a.ctl = cv.take<u64>(SL_WORDS);
  a.keep = cv.take<u32>(2 * (m + 1));
  a.val = cv.take<i64>(m + 1);
  a.st = cv.take<u32>(2 * (m + 1));
  a.rank = cv.take<u64>(m + 1);
  a.cval = cv.take<i64>(m + 1);
  a.cst = cv.take<u32>(2 * (m + 1));
  a.cline = cv.take<u64>(m + 1);
  void *scan_tmp = cv.take<uint8_t>(scan_bytes);
  HIPCHK(sidx_subs_plan(&a, scan_tmp, &scan_bytes, s), "subset slab launch");
  u64 w[SL_WORDS];
  HIPCHK(hipMemcpyAsync(w, a.ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
  HIPCHK(hipStreamSynchronize(s), "subset slab sync");
  if (w[SL_FLAGS])
    return set_msg(res, SHOCKIDX_EINVAL, "the carry does not allow this slab: its walk has ended or not begun, or its next line lies outside the slab");
  const u64 ke = w[SL_KE], nruns_call = w[SL_NCLOSED] + w[SL_FINAL];
  res->rows = ke;
  res->runs = nruns_call;
  if (ke > rows_cap) return set_msg(res, SHOCKIDX_ESPACE, "row capacity too small");
  if (nruns_call > runs_cap) return set_msg(res, SHOCKIDX_ESPACE, "run capacity too small");
  HIPCHK(sidx_subs_commit(&a, ke, w[SL_NCLOSED], s), "subset commit launch");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipStreamSynchronize(s), "subset slab sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms = ms;
  res->count = w[SL_COUNT];
  res->nruns = w[SL_NRUNS];
  res->size = w[SL_TOTSIZE];
  res->stop = (int32_t)w[SL_STOP];
  res->next_off = w[SL_NEXT_OFF];
  res->next_id = (int64_t)w[SL_NEXT_ID];
  res->total_ms = now_ms() - t0;
  const u32 code = (u32)w[SL_CODE];
  if (!code) return SHOCKIDX_OK;
  uint8_t txt[200];
  u64 k = 0;
  if (code == SUB_SYNTAX || code == SUB_RANGE) {
    k = w[SL_ERR_LEN] < 200 ? w[SL_ERR_LEN] : 200;  // enough for a 255-byte message
    if (k) {
      HIPCHK(hipMemcpyAsync(txt, (const uint8_t *)b.d_data + w[SL_ERR_OFF], k, hipMemcpyDeviceToHost, s), "text copy");
      HIPCHK(hipStreamSynchronize(s), "sync");
    }
  }
  return set_msg(res, SHOCKIDX_EFORMAT, subset_error_text(code, (i64)w[SL_ERR_V], (i64)w[SL_ERR_PREV], txt, k));
}

}  // extern "C"

// ---- Index read path: Idx.Part / Idx.Range (index/index.go:67-193) ------------------------
namespace {

// row i of the device table (16 bytes D2H); a row past the table reads as `dflt`
int read_row(shockidx_ctx *c, const void *d_rows, u64 nrows, u64 i, const u64 dflt[2], u64 out[2],
             Err res) {
  if (i >= nrows) {
    out[0] = dflt[0];
    out[1] = dflt[1];
    return 0;
  }
  HIPCHK(hipMemcpyAsync(out, (const u64 *)d_rows + 2 * i, 16, hipMemcpyDeviceToHost, c->stream), "row copy");
  HIPCHK(hipStreamSynchronize(c->stream), "row sync");
  return 0;
}

}  // namespace

extern "C" {

int shockidx_idx_part(shockidx_ctx *c, const void *d_rows, uint64_t nrows, const char *part, int64_t idx_length,
                      int64_t *pos, int64_t *length, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !part || !pos || !length) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  *pos = 0;
  *length = 0;
  const double t0 = now_ms();
  if (!d_rows) return set_msg(res, SHOCKIDX_EFORMAT, E_IDX_NOFILE);  // index.go:70-74
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  i64 a = 0, b = 0;
  const char *e = nullptr;
  const int kind = parse_part(part, idx_length, &a, &b, &e);
  if (kind < 0) return set_msg(res, SHOCKIDX_EFORMAT, e);
  // fresh zeroed records (index.go:88,94,109): a read past the file leaves zeros
  static const u64 zero[2] = {0, 0};
  u64 sr[2], er[2];
  if (int rc = read_row(c, d_rows, nrows, (u64)(a - 1), zero, sr, res)) return rc;
  if (kind == 0) {
    *pos = (i64)sr[0];
    *length = (i64)sr[1];
  } else {
    if (int rc = read_row(c, d_rows, nrows, (u64)(b - 1), zero, er, res)) return rc;
    *pos = (i64)sr[0];
    *length = (i64)(er[0] - sr[0] + er[1]);  // index.go:98-99 (int64 arithmetic wraps)
  }
  res->count = 1;
  res->total_ms = now_ms() - t0;
  return SHOCKIDX_OK;
}

int shockidx_idx_range(shockidx_ctx *c, const void *d_rows, uint64_t nrows, const char *part, int64_t idx_length,
                       void *d_recs, uint64_t recs_cap, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (!c || !part || (!d_recs && recs_cap)) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  const double t0 = now_ms();
  if (!d_rows) return set_msg(res, SHOCKIDX_EFORMAT, E_IDX_NOFILE);  // index.go:122-126
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  i64 a = 0, b = 0;
  const char *e = nullptr;
  const int kind = parse_part(part, idx_length, &a, &b, &e);
  if (kind < 0) return set_msg(res, SHOCKIDX_EFORMAT, e);
  const u64 a0 = (u64)(a - 1);
  if (kind == 0 || a == b) {  // one record (index.go:146-150, :185-191): rec starts zeroed
    static const u64 zero[2] = {0, 0};
    u64 r[2];
    if (int rc = read_row(c, d_rows, nrows, a0, zero, r, res)) return rc;
    res->count = 1;
    if (recs_cap < 1) return set_msg(res, SHOCKIDX_ESPACE, "record capacity too small");
    HIPCHK(hipMemcpyAsync(d_recs, r, 16, hipMemcpyHostToDevice, s), "rec copy");
    HIPCHK(hipStreamSynchronize(s), "rec sync");
    res->total_ms = now_ms() - t0;
    return SHOCKIDX_OK;
  }
  if (b < a) {  // the coalescing loop runs zero times: an empty list, no error
    res->total_ms = now_ms() - t0;
    return SHOCKIDX_OK;
  }
  const u64 nr = (u64)(b - a) + 1;
  if (nr > (u64)INT32_MAX) return set_msg(res, SHOCKIDX_EINVAL, "range too large for one call");
  size_t scan_bytes = 0;
  HIPCHK(sidx_scan_flags(nullptr, nullptr, nr, nullptr, &scan_bytes, s), "scan size");
  const u64 need = 12 * (nr + 64) + scan_bytes + 4096;
  if (int rc = c->d_sub.ensure(need, res)) return rc;
  Carver cv{c->d_sub};
  u32 *flags = cv.take<u32>(nr);
  u64 *id = cv.take<u64>(nr);
  void *scan_tmp = cv.take<uint8_t>(scan_bytes);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(sidx_range_flags((const u64 *)d_rows, nrows, a0, nr, flags, s), "range flags");
  HIPCHK(sidx_scan_flags(flags, id, nr, scan_tmp, &scan_bytes, s), "scan");
  u64 nrec = 0;
  if (int rc = scan_total(c, id, flags, nr, &nrec, res)) return rc;
  res->count = nrec;
  if (nrec > recs_cap) return set_msg(res, SHOCKIDX_ESPACE, "record capacity too small");
  HIPCHK(sidx_range_emit((const u64 *)d_rows, nrows, a0, nr, flags, id, (u64 *)d_recs, s), "range emit");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipStreamSynchronize(s), "range sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms = ms;
  res->total_ms = now_ms() - t0;
  return SHOCKIDX_OK;
}

}  // extern "C"
