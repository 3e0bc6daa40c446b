// sidx_stream.hpp -- control words and the first-failure key shared by the sectioned stream's kernels
// (sidx_stream.hip) and its entry point (sidx_stream_api.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"

namespace sidx {
enum StreamCtl : int {
  SS_INVALID = 0,  // a section outside the node
  SS_NOTHER = 1,   // sections the segmented path does not take (too long, or of no format under anonymize)
  SS_KEY = 2,      // FASTQ: min over failing (section, record, status), ~0: none; FASTA / SAM: the failing
                   //   item's section within the batch, ~0: none
  SS_KE = 3,       // items (records, sequences, lines) before the first failure
  SS_NCUT = 4,     // classify: batch starts after section 0
  SS_BAD = 5,      // FASTA / SAM: the first failing flat item (k_fa_anon_spans / k_sam_anon_spans), ~0: none
  SS_EOF = 6,      // SAM: k_sam_anon_spans' first line without '\n' (the segmented index emits none)
  SS_FMT0 = 7,     // classify: section 0's format when the segmented path takes it, else 0
  SS_NDELIV = 8,   // SAM: lines delivered before the first failure (blank and '@' lines deliver nothing)
  SS_WCOUNT = 9,   // SAM: k_sam_anon_write's own count (not read: SS_NDELIV is known before the write)
  SS_NWORDS = 16
};
// classify's batch starts: (section << 2) | its format (F_FASTA, F_FASTQ, F_SAM)
constexpr u32 SS_CUT_SHIFT = 2;
// (section within the batch, record within the section, ST_* status): sections in list order, then
// Read's order inside one.  A small section is at most SS_SMALL_MAX bytes and a record at least 8, so
// 24 bits hold the record.
constexpr u32 SS_SEC_SHIFT = 28;
constexpr u64 SS_REC_MASK = (1ull << 24) - 1;
constexpr u64 SS_SMALL_MAX = 16ull << 20;
__host__ __device__ inline u64 ss_key(u64 sec, u64 rec, u32 st) { return (sec << SS_SEC_SHIFT) | (rec << 4) | st; }
}  // namespace sidx
