// sidx_stream_api.cpp -- the sectioned download stream of the C ABI: request.Streamer.Stream with a
// Filter (request/streamer.go:78-98) over a list of sections of a node in HBM, over the kernels of
// sidx_stream.hip (the segmented index of FASTQ records, FASTA sequences and SAM lines) and
// sidx_filter.hip (spans, scan, writer).
//
// The section list is split, in list order, into groups: maximal runs of consecutive sections the
// segmented path takes in one format (at most that format's small-section limit long; FASTQ, FASTA or
// SAM as detected per section under anonymize, everything as FASTQ under fq2fa) -- one batch each, with
// no loop over its sections on the host and a fixed number of waits -- and single other sections (too
// long, or of no detected format), which go through the single-section filter (filter_section) from a
// 16-byte aligned copy.  shockidx_stream_last_stats reports how the last call's list was split.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_host.hpp"
#include "sidx_launch.hpp"
#include "sidx_stream.hpp"

using namespace sidx;
using namespace sidx_host;

namespace {

// Sections at most this long take the segmented path (SHOCKIDX_STREAM_SMALL, bytes).  The default is
// where the two paths were timed against each other ("The sectioned stream").
// Each format's default is the largest measured size at which 64 batched sections beat 64 single ones
// (2.8 KiB, 64 KiB and 1 MiB were measured for each format: 1 MiB for all three).
constexpr u64 STREAM_SMALL_DEFAULT = 1ull << 20;        // FASTQ: 1.47 against 42.2 ms (fq2fa)
constexpr u64 STREAM_SMALL_DEFAULT_FASTA = 1ull << 20;  // FASTA under anonymize: 1.87 against 26.2 ms
constexpr u64 STREAM_SMALL_DEFAULT_SAM = 1ull << 20;    // SAM under anonymize: 4.72 against 29.9 ms

// the environment's limit, when set, applies to every format; 0: everything takes the single-section path
u64 small_limit(int fmt) {
  u64 v = fmt == F_FASTA ? STREAM_SMALL_DEFAULT_FASTA : fmt == F_SAM ? STREAM_SMALL_DEFAULT_SAM : STREAM_SMALL_DEFAULT;
  if (const char *e = getenv("SHOCKIDX_STREAM_SMALL")) {
    char *end = nullptr;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end != e) v = x;
  }
  return v < SS_SMALL_MAX ? v : SS_SMALL_MAX;
}

struct Group {
  u64 lo, hi;    // sections [lo, hi) of the list
  bool batch;    // the segmented path; else one section through filter_section
  int fmt;       // the batch's format (F_FASTQ, F_FASTA, F_SAM)
  i64 pos, len;  // the single section
  u64 size;      // bytes it delivers (known after a sizing pass)
};

u64 round256(u64 v) { return (v + 255) / 256 * 256; }

// One batch of S small FASTA or SAM sections under anonymize: the flat items are the sequences
// fasta.Reader.Read delivers (every section's last one, which ends at the section end, is dropped) or the
// '\n'-terminated lines sam.Reader.Read reads; count = the sequences / the alignment lines delivered.
// The host waits, for either format: the item total (2), the first failure (1), the output total (2),
// the end (1) -- six, as for FASTQ.
int stream_batch_flat(shockidx_ctx *c, int fmt, const uint8_t *dd, u64 n, const uint8_t *d_secs, u64 S, uint8_t *d_out,
                      u64 out_cap, bool size_only, shockidx_subset_result *res, i64 *fail) {
  hipStream_t s = c->stream;
  const bool fasta = fmt == F_FASTA;
  size_t sb = 0;
  HIPCHK(sidx_scan_u64(nullptr, nullptr, S, nullptr, &sb, s), "scan size");
  if (int rc = c->d_cra.ensure(round256(8 * SS_NWORDS) + 2 * round256(8 * S) + sb + 4096, res)) return rc;
  Carver ca{c->d_cra};
  u64 *ctl = ca.take<u64>(SS_NWORDS);
  u64 *cnt = ca.take<u64>(S);
  u64 *base = ca.take<u64>(S);
  void *stmp = ca.take<uint8_t>(sb);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(hipMemsetAsync(ctl, 0xFF, 8 * SS_NWORDS, s), "memset");
  HIPCHK(hipMemsetAsync(ctl + SS_NDELIV, 0, 16, s), "memset");  // SS_NDELIV, SS_WCOUNT
  if (fasta) HIPCHK(sidx_stream_fa_count(dd, n, d_secs, S, cnt, s), "stream count");
  else HIPCHK(sidx_stream_sam_count(dd, n, d_secs, S, cnt, s), "stream count");
  HIPCHK(sidx_scan_u64(cnt, base, S, stmp, &sb, s), "scan");
  u64 K = 0;
  if (int rc = scan_total(c, base, cnt, S, &K, res)) return rc;
  size_t kb = 0;
  HIPCHK(sidx_scan_u64(nullptr, nullptr, K ? K : 1, nullptr, &kb, s), "scan size");
  if (int rc = c->d_sub.ensure(64 * (K + 8) + kb + 16 * 256 + 4096, res)) return rc;
  Carver cs{c->d_sub};
  u64 *rows = cs.take<u64>(2 * (K + 1));
  u32 *ord = cs.take<u32>(K + 1);
  u32 *rsec = cs.take<u32>(K + 1);
  u64 *span = cs.take<u64>(2 * (K + 1));
  u64 *outlen = cs.take<u64>(K + 1);
  u64 *outoff = cs.take<u64>(K + 1);
  void *ktmp = cs.take<uint8_t>(kb);
  if (fasta) {
    HIPCHK(sidx_stream_fa_emit(dd, n, d_secs, S, cnt, base, rows, ord, rsec, s), "stream index");
    HIPCHK(sidx_fa_anon_spans_seg(dd, n, rows, ord, K, span, outlen, ctl + SS_BAD, s), "anonymize spans");
  } else {
    HIPCHK(sidx_stream_sam_emit(dd, n, d_secs, S, cnt, base, rows, rsec, s), "stream index");
    HIPCHK(sidx_sam_anon_spans(dd, n, rows, K, span, outlen, ctl + SS_BAD, ctl + SS_EOF, s), "anonymize spans");
  }
  HIPCHK(sidx_stream_flat_finish(rsec, outlen, K, fasta ? 0 : 1, ctl, s), "stream finish");
  u64 w[SS_NWORDS];
  HIPCHK(hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
  HIPCHK(hipStreamSynchronize(s), "control sync");
  const u64 key = w[SS_KEY], Ke = w[SS_KE];  // the flat list is cut at the first failing item
  if (Ke > K || w[SS_EOF] != ~0ull || (key != ~0ull && key >= S))
    return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: stream item count");
  u64 total = 0;
  if (Ke) {
    HIPCHK(sidx_scan_u64(outlen, outoff, Ke, ktmp, &kb, s), "scan");
    if (int rc = scan_total(c, outoff, outlen, Ke, &total, res)) return rc;
  }
  res->count = fasta ? Ke : w[SS_NDELIV];
  res->size = total;
  if (!size_only) {
    if (total > out_cap) return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
    if (fasta) HIPCHK(sidx_fa_anon_write_seg(dd, n, span, outoff, ord, Ke, d_out, s), "anonymize write");
    else HIPCHK(sidx_sam_anon_write(dd, span, outlen, outoff, Ke, d_out, ctl + SS_WCOUNT, s), "anonymize write");
  }
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipStreamSynchronize(s), "stream sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms += ms;
  if (key == ~0ull) return SHOCKIDX_OK;
  *fail = (i64)key;
  return set_msg(res, SHOCKIDX_EFORMAT, fasta ? "Invalid fasta entry" : "sam alignment fields less than 11");
}

// One batch of S small sections of one format (d_secs: its first record).  res (reset by the caller):
// count / size delivered; OK, or EFORMAT with Read's text and *fail = the failing section within the
// batch.  FASTQ, the host waits: the record total (2), the first failure (1), the output total (2), the
// end (1) -- six per batch, for every format (stream_batch_flat).
int stream_batch(shockidx_ctx *c, int kind, int fmt, const uint8_t *dd, u64 n, const uint8_t *d_secs, u64 S,
                 uint8_t *d_out, u64 out_cap, bool size_only, shockidx_subset_result *res, i64 *fail) {
  hipStream_t s = c->stream;
  *fail = -1;
  if (fmt != F_FASTQ) return stream_batch_flat(c, fmt, dd, n, d_secs, S, d_out, out_cap, size_only, res, fail);
  size_t sb = 0;
  HIPCHK(sidx_scan_u64(nullptr, nullptr, S, nullptr, &sb, s), "scan size");
  if (int rc = c->d_cra.ensure(round256(8 * SS_NWORDS) + 2 * round256(8 * S) + sb + 4096, res)) return rc;
  Carver ca{c->d_cra};
  u64 *ctl = ca.take<u64>(SS_NWORDS);
  u64 *cnt = ca.take<u64>(S);
  u64 *base = ca.take<u64>(S);
  void *stmp = ca.take<uint8_t>(sb);
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(hipMemsetAsync(ctl, 0xFF, 8 * SS_NWORDS, s), "memset");
  HIPCHK(sidx_stream_count(dd, n, d_secs, S, cnt, s), "stream count");
  HIPCHK(sidx_scan_u64(cnt, base, S, stmp, &sb, s), "scan");
  u64 K = 0;
  if (int rc = scan_total(c, base, cnt, S, &K, res)) return rc;
  size_t kb = 0;
  HIPCHK(sidx_scan_u64(nullptr, nullptr, K ? K : 1, nullptr, &kb, s), "scan size");
  if (int rc = c->d_sub.ensure(64 * (K + 8) + kb + 16 * 256 + 4096, res)) return rc;
  Carver cs{c->d_sub};
  u64 *rows = cs.take<u64>(2 * (K + 1));
  u32 *ord = cs.take<u32>(K + 1);
  u32 *rsec = cs.take<u32>(K + 1);
  u32 *spans = cs.take<u32>(6 * (K + 1));
  u64 *outlen = cs.take<u64>(K + 1);
  u64 *outoff = cs.take<u64>(K + 1);
  void *ktmp = cs.take<uint8_t>(kb);
  u64 *unused_bad = cs.take<u64>(1);  // k_fq_spans' own first-bad word: k_ss_check made its checks already
  HIPCHK(sidx_stream_index(dd, n, d_secs, S, cnt, base, K, rows, ord, rsec, ctl, s), "stream index");
  u64 w[SS_NWORDS];
  HIPCHK(hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
  HIPCHK(hipStreamSynchronize(s), "control sync");
  const u64 key = w[SS_KEY], Ke = w[SS_KE];  // the flat list is cut at the first failing record
  if (Ke > K) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: stream record count");
  u64 total = 0;
  if (Ke) {
    HIPCHK(hipMemsetAsync(outlen, 0, 8 * Ke, s), "memset");
    HIPCHK(hipMemsetAsync(unused_bad, 0xFF, 8, s), "memset");
    HIPCHK(sidx_filter_spans(dd, n, rows, Ke, kind, spans, outlen, unused_bad, ord, s), "filter spans");
    HIPCHK(sidx_scan_u64(outlen, outoff, Ke, ktmp, &kb, s), "scan");
    if (int rc = scan_total(c, outoff, outlen, Ke, &total, res)) return rc;
  }
  res->count = Ke;
  res->size = total;
  if (!size_only) {
    if (total > out_cap) return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
    // the writer's block plan replaces the section-level words, which are spent
    const u64 nwf = total / sidx_filter_block() + 4;
    if (int rc = c->d_cra.ensure(8 * nwf + 256, res)) return rc;
    HIPCHK(sidx_filter_write(dd, n, rows, spans, outlen, outoff, Ke, total, kind, c->d_cra.as<u64>(), d_out, ord, s),
           "filter write");
  }
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipStreamSynchronize(s), "stream sync");
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ek0, c->ek1);
  res->kernel_ms += ms;
  if (key == ~0ull) return SHOCKIDX_OK;
  *fail = (i64)(key >> SS_SEC_SHIFT);
  const char *m = status_message((u32)(key & 15));
  return set_msg(res, SHOCKIDX_EFORMAT, m ? m : "internal error: stream status");
}

}  // namespace

extern "C" {

int shockidx_stream_filter_device(shockidx_ctx *c, const char *filter, const void *d_data, uint64_t n,
                                  const void *d_secs, uint64_t nsecs, void *d_out, uint64_t out_cap,
                                  int64_t *err_section, shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (err_section) *err_section = -1;
  if (!c || (!d_data && n) || ((uintptr_t)d_data & 15) || ((uintptr_t)d_out & 15) || (!d_out && out_cap) ||
      (!d_secs && nsecs) || ((uintptr_t)d_secs & 7))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  if (!filter || !*filter)  // the Streamer without a Filter (streamer.go:88-90): the plain gather
    return shockidx_subset_gather(c, d_data, n, d_secs, nsecs, d_out, out_cap, res);
  const int kind = filter_kind(filter);
  if (!kind) return set_msg(res, SHOCKIDX_EINVAL, "unknown filter");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  c->stream_stats = shockidx_stream_stats{};
  c->stream_stats.sections = nsecs;
  if (!nsecs) return SHOCKIDX_OK;
  const uint8_t *dd = (const uint8_t *)d_data, *secs = (const uint8_t *)d_secs;
  uint8_t *out = (uint8_t *)d_out;

  // every section checked against the node; the sections the segmented path does not take
  // and where a batch starts after section 0 (a list of small sections of one format: nowhere, so
  // nothing that grows with nsecs comes to the host)
  std::vector<u64> oth, cut;
  int fmt0 = 0;
  {
    if (int rc = c->d_cra.ensure(round256(8 * SS_NWORDS) + round256(4 * nsecs) + 2 * round256(8 * nsecs) + 4096, res))
      return rc;
    Carver ca{c->d_cra};
    u64 *ctl = ca.take<u64>(SS_NWORDS);
    int *fmt = ca.take<int>(nsecs);
    u64 *others = ca.take<u64>(nsecs);
    u64 *cuts = ca.take<u64>(nsecs);
    HIPCHK(hipMemsetAsync(ctl, 0, 8 * SS_NWORDS, s), "memset");
    // anonymize reads through multi.Reader, once per section (multi.go:43-62); fq2fa does not detect
    if (kind == 2) HIPCHK(sidx_launch_detect_sections(dd, n, secs, nsecs, fmt, s), "detect launch");
    HIPCHK(sidx_stream_classify(secs, nsecs, n, kind == 2 ? fmt : nullptr, small_limit(F_FASTQ), small_limit(F_FASTA),
                                small_limit(F_SAM), ctl, others, cuts, s),
           "classify");
    u64 w[SS_NWORDS];
    HIPCHK(hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
    HIPCHK(hipStreamSynchronize(s), "control sync");
    if (w[SS_INVALID]) return set_msg(res, SHOCKIDX_EINVAL, "section exceeds the data");
    if (w[SS_NOTHER] > nsecs || w[SS_NCUT] > nsecs) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: stream groups");
    fmt0 = (int)w[SS_FMT0];
    oth.resize(w[SS_NOTHER]);
    cut.resize(w[SS_NCUT]);
    if (!oth.empty()) HIPCHK(hipMemcpyAsync(oth.data(), others, 8 * oth.size(), hipMemcpyDeviceToHost, s), "list copy");
    if (!cut.empty()) HIPCHK(hipMemcpyAsync(cut.data(), cuts, 8 * cut.size(), hipMemcpyDeviceToHost, s), "list copy");
    if (!oth.empty() || !cut.empty()) {
      HIPCHK(hipStreamSynchronize(s), "list sync");
      std::sort(oth.begin(), oth.end());
      std::sort(cut.begin(), cut.end());
    }
  }
  std::vector<Group> groups;
  {
    std::vector<i64> osec(2 * oth.size());
    for (size_t k = 0; k < oth.size(); ++k)
      HIPCHK(hipMemcpyAsync(&osec[2 * k], secs + 16 * oth[k], 16, hipMemcpyDeviceToHost, s), "section copy");
    if (!oth.empty()) HIPCHK(hipStreamSynchronize(s), "section sync");
    // the singles and the batch starts (section 0 when the segmented path takes it, then the cuts), merged
    // in list order; a batch runs to the next of either
    size_t io = 0, ic = 0;
    u64 at = 0;
    while (at < nsecs) {
      if (io < oth.size() && oth[io] == at) {
        groups.push_back(Group{at, at + 1, false, 0, osec[2 * io], osec[2 * io + 1], 0});
        ++io;
        ++at;
        continue;
      }
      int f = 0;
      if (at == 0) f = fmt0;
      else if (ic < cut.size() && (cut[ic] >> SS_CUT_SHIFT) == at) f = (int)(cut[ic++] & ((1u << SS_CUT_SHIFT) - 1));
      if (f != F_FASTQ && f != F_FASTA && f != F_SAM) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: stream groups");
      u64 hi = nsecs;
      if (io < oth.size() && oth[io] < hi) hi = oth[io];
      if (ic < cut.size() && (cut[ic] >> SS_CUT_SHIFT) < hi) hi = cut[ic] >> SS_CUT_SHIFT;
      if (hi <= at) return set_msg(res, SHOCKIDX_EINTERNAL, "internal error: stream groups");
      groups.push_back(Group{at, hi, true, f, 0, 0, 0});
      c->stream_stats.batches += 1;
      c->stream_stats.batched += hi - at;
      c->stream_stats.by_format[f == F_FASTQ ? 0 : f == F_FASTA ? 1 : 2] += 1;
      at = hi;
    }
    c->stream_stats.singles = oth.size();
  }

  // The groups in list order, stopping after the first section whose status is not OK.  A group
  // whose output does not start on a 16-byte boundary of d_out is written to c->d_sec and copied.
  i64 esec = -1;
  u64 done_count = 0, done_size = 0;
  double kernel_ms = 0;
  auto walk = [&](bool size_only) -> int {
    u64 off = 0, cnt = 0;
    esec = -1;
    int status = SHOCKIDX_OK;
    for (Group &g : groups) {
      shockidx_subset_result r;
      reset_result(&r);
      uint8_t *dst = nullptr;
      u64 cap = 0;
      const u64 in_bytes = g.batch ? 0 : round256((u64)g.len + 64);
      const bool staged = !size_only && (off & 15) != 0;
      if (!g.batch || staged)
        if (int rc = c->d_sec.ensure(in_bytes + (staged ? g.size + 64 : 0) + 64, res)) return rc;
      if (staged) {
        dst = c->d_sec.as<uint8_t>() + in_bytes;
        cap = g.size;
      } else if (!size_only) {
        dst = out ? out + off : nullptr;
        cap = out_cap > off ? out_cap - off : 0;
      }
      int rc;
      i64 fail = -1;
      if (g.batch) {
        rc = stream_batch(c, kind, g.fmt, dd, n, secs + 16 * g.lo, g.hi - g.lo, dst, cap, size_only, &r, &fail);
      } else {
        if (g.len)
          HIPCHK(hipMemcpyAsync(c->d_sec.as<uint8_t>(), dd + g.pos, (size_t)g.len, hipMemcpyDeviceToDevice, s),
                 "section copy");
        rc = filter_section(c, kind, c->d_sec.as<uint8_t>(), (u64)g.len, dst, cap, &r, size_only);
        fail = 0;
      }
      kernel_ms += r.kernel_ms;
      if (rc != SHOCKIDX_OK && rc != SHOCKIDX_EFORMAT) {
        forward_error(res, r, rc);
        res->count = cnt + r.count;  // ESPACE (one group, so no sizing pass came first): what the call needs
        res->size = off + r.size;
        return rc;
      }
      if (staged && r.size)
        HIPCHK(hipMemcpyAsync(out + off, dst, r.size, hipMemcpyDeviceToDevice, s), "output copy");
      if (size_only) g.size = r.size;
      off += r.size;
      cnt += r.count;
      if (rc == SHOCKIDX_EFORMAT) {  // Streamer.ESection (streamer.go:92-95)
        esec = (i64)g.lo + fail;
        status = forward_error(res, r, rc);
        break;
      }
    }
    done_count = cnt;
    done_size = off;
    return status;
  };
  int rc = SHOCKIDX_OK;
  if (groups.size() > 1) {  // nothing may be written when the whole stream does not fit: size it first
    rc = walk(true);
    if (rc < 0) return rc;
    if (done_size > out_cap) {
      res->count = done_count;
      res->size = done_size;
      return set_msg(res, SHOCKIDX_ESPACE, "output capacity too small");
    }
    res->err_len = 0;
    res->err[0] = 0;
  }
  rc = walk(false);
  if (rc < 0) return rc;
  HIPCHK(hipStreamSynchronize(s), "stream sync");
  res->status = rc;
  res->count = done_count;
  res->size = done_size;
  res->kernel_ms = kernel_ms;
  res->total_ms = now_ms() - t0;
  if (err_section) *err_section = esec;
  return rc;
}

int shockidx_stream_last_stats(const shockidx_ctx *c, shockidx_stream_stats *out) {
  if (!c || !out) return SHOCKIDX_EINVAL;
  *out = c->stream_stats;
  return SHOCKIDX_OK;
}

}  // extern "C"
