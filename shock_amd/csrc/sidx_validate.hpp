// sidx_validate.hpp -- one record of each format checked the way the reference's readers check it,
// templated on the byte accessor (sidx_device.hpp), and the row count of an input no record ends
// early.  Shared by the index build (sidx_kernels.hip) and the batch build (sidx_batch.hip): both
// call these functions, so their statuses, lengths and counts cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"
#include "sidx_device.hpp"

namespace sidx {

constexpr u64 INF = ~0ull;

// ====================================================================================
// Validators (one record; templated on the accessor).  Return ST_*; set len on ST_OK.
// ====================================================================================
__device__ __forceinline__ u32 fr_to_st(u32 r) { return r == FR_DEFER ? ST_DEFER : ST_NEEDMORE; }

// fastq.go:134-213 for the group (record) starting at s.
template <class A>
__device__ u32 fastq_record(A &a, u64 s, u64 &len) {
  u64 e0, e1, e2, e3;
  u32 r;
  if (s >= a.end) return a.eof ? ST_END : ST_NEEDMORE;  // id line absent: (0, EOF)
  r = a.find(C_NL, s, INF, e0);
  if (r >= FR_DEFER) return fr_to_st(r);
  if (r == FR_NONE) return ST_FQ_TRUNC;  // non-empty id line without '\n' at EOF (:154-156)
  if (e0 == s) {                          // blank line where an id line is due (:143-152)
    // a group whose 4 preceding bytes are all '\n' follows another blank group: only the
    // first group of a blank run can be the terminating one (keeps the scans linear)
    if ((s >= 4 || a.front >= 4) && a.byte(s - 1) == '\n' && a.byte(s - 2) == '\n' &&
        a.byte(s - 3) == '\n' && a.byte(s - 4) == '\n')
      return ST_DONTCARE;
    u64 y, z;
    r = a.find(C_NOTNL, s, INF, y);
    if (r >= FR_DEFER) return fr_to_st(r);
    if (r == FR_NONE) return ST_END;  // only blank lines up to EOF (:154-158, len 0)
    r = a.find(C_NL, y, INF, z);
    if (r >= FR_DEFER) return fr_to_st(r);
    return r == FR_FOUND ? ST_FQ_EMPTYLINES : ST_FQ_TRUNC;  // (:161-163) / (:154-156)
  }
  if (a.byte(s) != '@') return ST_FQ_NOAT;   // :164-166
  if (e0 - s == 1) return ST_FQ_NOID;        // "@\n" (:167-169)
  r = a.find(C_NL, e0 + 1, INF, e1);         // sequence line (:173-182)
  if (r >= FR_DEFER) return fr_to_st(r);
  if (r == FR_NONE) return ST_FQ_TRUNC;
  if (e1 == e0 + 1) return ST_FQ_EMPTYSEQ;
  r = a.find(C_NL, e1 + 1, INF, e2);         // plus line (:185-199)
  if (r >= FR_DEFER) return fr_to_st(r);
  if (r == FR_NONE) return ST_FQ_TRUNC;
  if (a.byte(e1 + 1) != '+') return ST_FQ_NOPLUS;
  u64 plo, phi;
  trim_space(a, e1 + 1, e2 + 1, plo, phi);
  if (phi - plo > 1) {
    u64 ilo, ihi;
    trim_space(a, s + 1, e0 + 1, ilo, ihi);
    if (ihi - ilo != phi - plo - 1) return ST_FQ_IDMISMATCH;
    for (u64 k = 0; k < ihi - ilo; ++k)
      if (a.byte(ilo + k) != a.byte(plo + 1 + k)) return ST_FQ_IDMISMATCH;
  }
  r = a.find(C_NL, e2 + 1, INF, e3);         // quality line (:202-209), EOF tolerated
  if (r >= FR_DEFER) return fr_to_st(r);
  const u64 qend = (r == FR_FOUND) ? e3 + 1 : a.end;
  u64 slo, shi, qlo, qhi;
  trim_space(a, e0 + 1, e1 + 1, slo, shi);
  trim_space(a, e2 + 1, qend, qlo, qhi);
  if (shi - slo != qhi - qlo) return ST_FQ_LENMISMATCH;
  len = qend - s;                            // :211
  return ST_OK;
}

// fasta.go:111-121: piece [lo, hi) (its '>' excluded) is valid iff TrimSpace of it holds a
// '\n' (Split(...)[1:] joined non-empty).
template <class A>
__device__ u32 fasta_piece_ok(A &a, u64 lo, u64 hi, bool &ok) {
  u64 tl, th, q;
  trim_space(a, lo, hi, tl, th);
  if (th <= tl) { ok = false; return FR_FOUND; }
  const u32 r = a.find(C_NL, tl, th, q);
  if (r >= FR_DEFER) return r;
  ok = (r == FR_FOUND);
  return FR_FOUND;
}

// fasta.go:93-140 for the record starting at rs; the scan for '>' starts at lo (one past
// the '>' that precedes it, or 0 for a file not starting with '>').
template <class A>
__device__ u32 fasta_record(A &a, u64 rs, u64 lo, u64 &len, u64 &epos, u64 &elen) {
  if (rs >= a.end) return a.eof ? ST_ABSENT : ST_NEEDMORE;
  for (;;) {
    u64 g, q;
    u32 r = a.find(C_X, lo, INF, g);
    if (r >= FR_DEFER) return fr_to_st(r);
    if (r == FR_NONE) {  // EOF piece [lo, end): validated iff len > 1 && holds '\n' (:111)
      if (a.end - lo > 1) {
        r = a.find(C_NL, lo, a.end, q);
        if (r >= FR_DEFER) return fr_to_st(r);
        if (r == FR_FOUND) {
          bool ok;
          r = fasta_piece_ok(a, lo, a.end, ok);
          if (r >= FR_DEFER) return fr_to_st(r);
          if (!ok) { epos = lo; elen = a.end - lo; return ST_FA_INVALID; }
        }
      }
      len = a.end - rs;  // :123-125
      return ST_OK;
    }
    r = a.find(C_NL, lo, g, q);  // '\n' since the previous '>' -> record boundary
    if (r >= FR_DEFER) return fr_to_st(r);
    if (r == FR_FOUND) {
      bool ok;
      r = fasta_piece_ok(a, lo, g, ok);
      if (r >= FR_DEFER) return fr_to_st(r);
      if (!ok) { epos = lo; elen = g + 1 - lo; return ST_FA_INVALID; }  // piece incl. '>'
      len = g - rs;  // :126-128 (UnreadByte)
      return ST_OK;
    }
    lo = g + 1;  // embedded '>' (:131-132)
  }
}

// sam.go:83-98 for the record starting at s.
template <class A>
__device__ u32 sam_record(A &a, u64 s, u64 &len) {
  if (s >= a.end) return a.eof ? ST_ABSENT : ST_NEEDMORE;
  u64 p = s;
  for (;;) {
    u64 q;
    const u32 r = a.find(C_NL, p, INF, q);
    if (r >= FR_DEFER) return fr_to_st(r);
    if (r == FR_NONE) { len = a.end - s; return ST_OK; }  // last line / leftover
    if (q > p && a.byte(p) != '@') { len = q + 1 - s; return ST_OK; }  // terminator line
    p = q + 1;
    if (p >= a.end) {
      if (!a.eof) return ST_NEEDMORE;
      len = a.end - s;
      return ST_OK;
    }
  }
}

// line.go:37-45 for the line starting at s (always a row, possibly empty at EOF).
template <class A>
__device__ u32 line_record(A &a, u64 s, u64 &len) {
  u64 q;
  const u32 r = a.find(C_NL, s, INF, q);
  if (r >= FR_DEFER) return fr_to_st(r);
  len = (r == FR_FOUND) ? q + 1 - s : a.end - s;
  return ST_OK;
}

template <int F, class A>
__device__ __forceinline__ u32 run_record(A &a, u64 s, u64 aux, u64 &len, u64 &epos, u64 &elen) {
  if (F == F_FASTQ) return fastq_record(a, s, len);
  if (F == F_FASTA) return fasta_record(a, s, aux, len, epos, elen);
  if (F == F_SAM) return sam_record(a, s, len);
  return line_record(a, s, len);
}

// The rows of an input whose final monoid state is fin when no record terminates it early: FASTQ
// groups 0..T/4, FASTA records 0..B, SAM records 0..Tterm, lines 0..T.
__device__ __forceinline__ u64 natural_count(int fmt, u64 fin) {
  if (fmt == F_FASTQ) return (fin >> 2) + 1;
  if (fmt == F_FASTA) return (fin >> 1) + 1;
  if (fmt == F_SAM) return (fin >> 2) + 1;
  return fin + 1;
}

}  // namespace sidx
