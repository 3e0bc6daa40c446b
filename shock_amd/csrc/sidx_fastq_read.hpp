// sidx_fastq_read.hpp -- fastq.Reader.Read (fastq.go:50-132) restated for the device, shared by the
// download filters (sidx_filter.hip) and the sectioned stream (sidx_stream.hip): the plain byte
// accessor, the first three line ends of a record, and Read's checks in Read's order over an accessor.
#pragma once
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"
#include "sidx_device.hpp"

namespace sidx {

constexpr u64 NOLIM = ~0ull;

struct GAcc {  // plain global-memory byte view for trim_space
  const uint8_t *g;
  __device__ __forceinline__ u32 byte(u64 p) const { return g[p]; }
  __device__ __forceinline__ const uint8_t *ptr() const { return g; }
  __device__ __forceinline__ u64 base() const { return 0; }
};

// The first three '\n' of the record [off, end) (the caller guarantees they exist inside it); n: the
// readable bytes of data.
__device__ __forceinline__ void first3_nl(const uint8_t *data, u64 n, u64 off, u64 end, u64 &e0, u64 &e1, u64 &e2) {
  u32 found = 0;
  // SIDX_SP_BATCH x 16 bytes per step, the loads issued together (one load per step cost a memory round
  // trip per 16 bytes: 6.1 ms per 10 GiB section)
#ifndef SIDX_SP_BATCH
#define SIDX_SP_BATCH 4  // 16-byte loads issued together per step (4: 11.8 ms fq2fa, 8: 12.0, 16: 12.7)
#endif
  for (u64 b0 = off & ~15ull; b0 < end && found < 3; b0 += 16 * SIDX_SP_BATCH) {
    uint4 v[SIDX_SP_BATCH];
#pragma unroll
    for (int k = 0; k < SIDX_SP_BATCH; ++k) {
      const u64 b = b0 + 16 * (u64)k;
      v[k] = (b + 16 <= n) ? load16(data + b) : (b < n ? load16_partial(data, b, n) : make_uint4(0, 0, 0, 0));
    }
#pragma unroll
    for (int k = 0; k < SIDX_SP_BATCH; ++k) {
      const u64 b = b0 + 16 * (u64)k;
      u32 m = b < end ? eq16(v[k], '\n') : 0u;
      if (b < off) m &= ~0u << (u32)(off - b);
      while (m && found < 3) {
        const u64 pos = b + (u64)__builtin_ctz(m);
        if (pos >= end) break;
        if (found == 0) e0 = pos;
        else if (found == 1) e1 = pos;
        else e2 = pos;
        ++found;
        m &= m - 1;
      }
    }
  }
}

// fastq.go:50-132 Reader.Read for the record at s (one wave; WaveAcc scans cooperatively).
// Returns ST_OK / ST_END (no record: only blank lines or nothing left) or the error status.
template <class A>
__device__ u32 fastq_read_status(A &a, u64 s) {
  u64 e0, e1, e2, e3;
  u32 r;
  if (s >= a.end) return ST_END;                // ReadBytes -> ("", EOF)  (:56-66)
  r = a.find(C_NL, s, NOLIM, e0);
  if (r == FR_NONE) return ST_FQ_TRUNC;         // non-empty id line at EOF (:68-72)
  if (e0 == s) {                                // blank lines: skipped only up to EOF
    u64 y, z;
    r = a.find(C_NOTNL, s, NOLIM, y);
    if (r == FR_NONE) return ST_END;
    r = a.find(C_NL, y, NOLIM, z);
    return r == FR_FOUND ? ST_FQ_EMPTYLINES : ST_FQ_TRUNC;  // (:76-78) / (:68-72)
  }
  if (a.byte(s) != '@') return ST_FQ_NOAT;      // :79-81
  u64 ilo, ihi;
  trim_space(a, s + 1, e0 + 1, ilo, ihi);
  if (ihi == ilo) return ST_FQ_NOID;            // :83-87
  r = a.find(C_NL, e0 + 1, NOLIM, e1);            // :89-95
  if (r == FR_NONE) return ST_FQ_TRUNC;
  u64 slo, shi;
  trim_space(a, e0 + 1, e1 + 1, slo, shi);
  if (shi == slo) return ST_FQ_EMPTYSEQ;        // :96-100
  r = a.find(C_NL, e1 + 1, NOLIM, e2);            // :102-110
  if (r == FR_NONE) return ST_FQ_TRUNC;
  if (a.byte(e1 + 1) != '+') return ST_FQ_NOPLUS;
  u64 plo, phi;
  trim_space(a, e1 + 1, e2 + 1, plo, phi);      // :111-115
  if (phi - plo > 1) {
    if (ihi - ilo != phi - plo - 1) return ST_FQ_IDMISMATCH;
    for (u64 k = 0; k < ihi - ilo; ++k)
      if (a.byte(ilo + k) != a.byte(plo + 1 + k)) return ST_FQ_IDMISMATCH;
  }
  r = a.find(C_NL, e2 + 1, NOLIM, e3);            // :117-126, EOF tolerated
  const u64 qend = (r == FR_FOUND) ? e3 + 1 : a.end;
  u64 qlo, qhi;
  trim_space(a, e2 + 1, qend, qlo, qhi);
  if (shi - slo != qhi - qlo) return ST_FQ_LENMISMATCH;
  return ST_OK;
}

}  // namespace sidx
