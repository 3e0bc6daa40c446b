// sidx_plan_api.cpp -- shockidx_download_plan: every part of a ?download&index=X&part=... request
// (controller/node/single.go:372-483) turned into the Streamer's section list in device memory,
// over the kernels of sidx_plan.hip.  The part strings, SizePart and the order of the errors are
// host arithmetic (sidx_plan_host.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/shockidx.h"
#include "sidx_common.hpp"
#include "sidx_plan.hpp"
#include "sidx_plan_host.hpp"
#include "sidx_launch.hpp"
#include "sidx_host.hpp"

using namespace sidx;
using namespace sidx_host;

namespace {

struct Plan {
  shockidx_ctx *c;
  shockidx_subset_result *res;
  int64_t *err_part;
  double t0;
};

int plan_fail(const Plan &p, int64_t part, const char *text) {
  if (p.err_part) *p.err_part = part;
  p.res->total_ms = now_ms() - p.t0;
  return set_msg(p.res, SHOCKIDX_EFORMAT, text);
}
int plan_done(const Plan &p, u64 count, u64 size) {
  p.res->count = count;
  p.res->size = size;
  p.res->total_ms = now_ms() - p.t0;
  return SHOCKIDX_OK;
}
int plan_short(const Plan &p, u64 need) {
  p.res->count = need;
  p.res->total_ms = now_ms() - p.t0;
  return set_msg(p.res, SHOCKIDX_ESPACE, "section capacity too small");
}
void kernel_time(const Plan &p) {
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, p.c->ek0, p.c->ek1);
  p.res->kernel_ms = ms;
}

// SIZE: SizePart per part on the host (virtual.go:50-80; the empty-node check of single.go:463-466
// is the controller's), the sections uploaded
int plan_size(const Plan &p, const char *const *parts, u64 nparts, i64 file_size, i64 chunk_size, void *d_secs,
              u64 secs_cap) {
  shockidx_subset_result *res = p.res;
  std::vector<i64> secs(2 * nparts);
  u64 size = 0;
  for (u64 k = 0; k < nparts; ++k) {
    const char *e = nullptr;
    if (sidx_plan::size_part(parts[k], file_size, chunk_size, &secs[2 * k], &secs[2 * k + 1], &e) < 0)
      return plan_fail(p, (int64_t)k, e);
    size += (u64)secs[2 * k + 1];
  }
  if (nparts > secs_cap) return plan_short(p, nparts);
  HIPCHK(hipMemcpyAsync(d_secs, secs.data(), 16 * nparts, hipMemcpyHostToDevice, p.c->stream), "section copy");
  HIPCHK(hipStreamSynchronize(p.c->stream), "plan sync");
  return plan_done(p, nparts, size);
}

// PART: one kernel over the parts, one wait (the size)
int plan_part(const Plan &p, const sidx_plan::Parsed &pp, const void *d_rows, u64 nrows, void *d_secs, u64 secs_cap) {
  shockidx_ctx *c = p.c;
  shockidx_subset_result *res = p.res;
  hipStream_t s = c->stream;
  const u64 P = pp.segs.size();
  if (P > secs_cap) return plan_short(p, P);
  if (int rc = c->d_sub.ensure(8 * PC_NWORDS + 16 * (P + 64) + 4096, res)) return rc;
  Carver cv{c->d_sub};
  u64 *ctl = cv.take<u64>(PC_NWORDS);
  u64 *ab = cv.take<u64>(2 * P);
  std::vector<u64> h(2 * P);
  for (u64 k = 0; k < P; ++k) {
    h[k] = pp.segs[k].a0;
    h[P + k] = pp.segs[k].b0;
  }
  HIPCHK(hipMemcpyAsync(ab, h.data(), 16 * P, hipMemcpyHostToDevice, s), "part copy");
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(sidx_plan_init(ctl, s), "plan init");
  HIPCHK(sidx_plan_part((const u64 *)d_rows, nrows, ab, ab + P, P, (u64 *)d_secs, ctl + PC_SIZE, s), "plan part");
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  u64 size = 0;
  if (int rc = d2h(c, &size, ctl + PC_SIZE, res)) return rc;
  kernel_time(p);
  return plan_done(p, P, size);
}

// RANGE and CHUNK_RANGE.  RANGE: the flag, scan, total and two emit passes over all parts' visits,
// the capacity checked on the device, one wait (count and size).  CHUNK_RANGE: the same into the
// workspace (the matrix records, each with its part), their level-2 segments and visit total, one
// wait (the error key, the segment count, the visit total), then the passes again over the record
// index into d_secs and the second wait.
int plan_range(const Plan &p, const sidx_plan::Parsed &pp, bool chunk, const void *d_rows, u64 nrows,
               const void *d_rec_rows, u64 rec_nrows, i64 rec_length, void *d_secs, u64 secs_cap) {
  shockidx_ctx *c = p.c;
  shockidx_subset_result *res = p.res;
  hipStream_t s = c->stream;
  const u64 P = pp.segs.size(), V = pp.visits;
  size_t scan_bytes = 0, scan64 = 0;
  HIPCHK(sidx_scan_flags(nullptr, nullptr, V, nullptr, &scan_bytes, s), "scan size");
  HIPCHK(sidx_scan_u64(nullptr, nullptr, V, nullptr, &scan64, s), "scan size");
  // level 1: a0[P] off[P + 1] | flags vseg id | scan; CHUNK_RANGE: recs part a02 nr2 off2 | scan
  const u64 need = 8 * PC_NWORDS + 16 * (P + 64) + 16 * (V + 64) + scan_bytes + (chunk ? 44 * (V + 64) + scan64 : 0) + 8192;
  if (int rc = c->d_sub.ensure(need, res)) return rc;
  Carver cv{c->d_sub};
  u64 *ctl = cv.take<u64>(PC_NWORDS);
  u64 *seg = cv.take<u64>(2 * P + 1);
  u32 *flags = cv.take<u32>(V), *vseg = cv.take<u32>(V);
  u64 *id = cv.take<u64>(V);
  void *scan_tmp = cv.take<uint8_t>(scan_bytes);
  std::vector<u64> h(2 * P + 1);
  u64 off = 0;
  for (u64 k = 0; k < P; ++k) {
    h[k] = pp.segs[k].a0;
    h[P + k] = off;
    off += pp.segs[k].nr;
  }
  h[2 * P] = off;
  HIPCHK(hipMemcpyAsync(seg, h.data(), 8 * (2 * P + 1), hipMemcpyHostToDevice, s), "part copy");
  HIPCHK(hipEventRecord(c->ek0, s), "event");
  HIPCHK(sidx_plan_init(ctl, s), "plan init");
  u64 w[PC_NWORDS];
  if (!chunk) {
    HIPCHK(sidx_plan_level((const u64 *)d_rows, nrows, seg, seg + P, P, V, flags, vseg, id, scan_tmp, &scan_bytes, ctl,
                           PC_NSEC, secs_cap, (u64 *)d_secs, nullptr, nullptr, ctl + PC_SIZE, s),
           "plan level");
  } else {
    u64 *recs = cv.take<u64>(2 * V);
    u32 *rpart = cv.take<u32>(V);
    u64 *a02 = cv.take<u64>(V), *nr2 = cv.take<u64>(V), *off2 = cv.take<u64>(V);
    void *tmp64 = cv.take<uint8_t>(scan64);
    HIPCHK(sidx_plan_level((const u64 *)d_rows, nrows, seg, seg + P, P, V, flags, vseg, id, scan_tmp, &scan_bytes, ctl,
                           PC_N1, V, recs, rpart, nullptr, nullptr, s),
           "plan level 1");
    HIPCHK(sidx_plan_segments(recs, rpart, V, ctl, rec_length, a02, nr2, off2, tmp64, &scan64, s), "plan segments");
    HIPCHK(hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
    HIPCHK(hipStreamSynchronize(s), "plan sync");
    const sidx_plan::PlanError e = sidx_plan::first_error(pp, w[PC_ERRKEY], -1);
    if (e.part >= 0) return plan_fail(p, e.part, e.text);
    const u64 N1 = w[PC_N1], V2 = w[PC_V2];
    if (V2 > sidx_plan::MAX_VISITS) return set_msg(res, SHOCKIDX_EINVAL, "plan too large for one call");
    if (!V2) {
      HIPCHK(hipEventRecord(c->ek1, s), "event");
      return plan_done(p, 0, 0);
    }
    size_t scan2 = 0;
    HIPCHK(sidx_scan_flags(nullptr, nullptr, V2, nullptr, &scan2, s), "scan size");
    if (int rc = c->d_plan.ensure(16 * (V2 + 64) + scan2 + 4096, res)) return rc;
    Carver c2{c->d_plan};
    u32 *flags2 = c2.take<u32>(V2), *vseg2 = c2.take<u32>(V2);
    u64 *id2 = c2.take<u64>(V2);
    void *tmp2 = c2.take<uint8_t>(scan2);
    HIPCHK(sidx_plan_level((const u64 *)d_rec_rows, rec_nrows, a02, off2, N1, V2, flags2, vseg2, id2, tmp2, &scan2, ctl,
                           PC_NSEC, secs_cap, (u64 *)d_secs, nullptr, nullptr, ctl + PC_SIZE, s),
           "plan level 2");
  }
  HIPCHK(hipEventRecord(c->ek1, s), "event");
  HIPCHK(hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s), "control copy");
  HIPCHK(hipStreamSynchronize(s), "plan sync");
  kernel_time(p);
  if (w[PC_NSEC] > secs_cap) return plan_short(p, w[PC_NSEC]);
  return plan_done(p, w[PC_NSEC], w[PC_SIZE]);
}

}  // namespace

extern "C" int shockidx_download_plan(shockidx_ctx *c, int mode, const char *const *parts, uint64_t nparts,
                                      const void *d_rows, uint64_t nrows, int64_t idx_length, const void *d_rec_rows,
                                      uint64_t rec_nrows, int64_t rec_length, int64_t file_size, int64_t chunk_size,
                                      void *d_secs, uint64_t secs_cap, int64_t *err_part,
                                      shockidx_subset_result *res) {
  shockidx_subset_result tmp;
  if (!res) res = &tmp;
  reset_result(res);
  if (err_part) *err_part = -1;
  if (!c || mode < SHOCKIDX_PLAN_PART || mode > SHOCKIDX_PLAN_SIZE || (!parts && nparts) || (!d_secs && secs_cap) ||
      ((uintptr_t)d_rows & 15) || ((uintptr_t)d_rec_rows & 15) || ((uintptr_t)d_secs & 7))
    return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  for (u64 k = 0; k < nparts; ++k)
    if (!parts[k]) return set_msg(res, SHOCKIDX_EINVAL, "invalid argument");
  if (nparts > sidx_plan::MAX_PARTS) return set_msg(res, SHOCKIDX_EINVAL, "too many parts for one call");
  const Plan p = {c, res, err_part, now_ms()};
  if (!nparts) return plan_done(p, 0, 0);  // ("requires part parameter" is the controller's)
  HIPCHK(hipSetDevice(c->device), "hipSetDevice");
  if (mode == SHOCKIDX_PLAN_SIZE) return plan_size(p, parts, nparts, file_size, chunk_size, d_secs, secs_cap);
  // os.Open comes before the part is parsed (index.go:70-74, :122-126)
  if (!d_rows) return plan_fail(p, 0, sidx_plan::E_IDX_NOFILE);
  const sidx_plan::Parsed pp = sidx_plan::parse_parts(parts, nparts, idx_length);
  const bool chunk = mode == SHOCKIDX_PLAN_CHUNK_RANGE;
  if (!chunk || !pp.visits || !d_rec_rows) {  // no level 2 runs: the host knows the error
    const sidx_plan::PlanError e = sidx_plan::first_error(pp, ~0ull, chunk && !d_rec_rows ? pp.first_nonempty : -1);
    if (e.part >= 0) return plan_fail(p, e.part, e.text);
  }
  if (mode == SHOCKIDX_PLAN_PART) return plan_part(p, pp, d_rows, nrows, d_secs, secs_cap);
  if (pp.visits > sidx_plan::MAX_VISITS) return set_msg(res, SHOCKIDX_EINVAL, "plan too large for one call");
  if (!pp.visits) return plan_done(p, 0, 0);
  return plan_range(p, pp, chunk, d_rows, nrows, d_rec_rows, rec_nrows, rec_length, d_secs, secs_cap);
}
