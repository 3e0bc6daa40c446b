// sidx_stream.hpp -- control words and the first-failure key shared by the sectioned stream's kernels
// (sidx_stream.hip) and its entry point (sidx_stream_api.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"

namespace sidx {
enum StreamCtl : int {
  SS_INVALID = 0,  // a section outside the node
  SS_NOTHER = 1,   // sections the segmented path does not take (too long, or not FASTQ under anonymize)
  SS_KEY = 2,      // min over failing (section, record, status), ~0: none
  SS_KE = 3,       // records delivered before it
  SS_NWORDS = 8
};
// (section within the batch, record within the section, ST_* status): sections in list order, then
// Read's order inside one.  A small section is at most SS_SMALL_MAX bytes and a record at least 8, so
// 24 bits hold the record.
constexpr u32 SS_SEC_SHIFT = 28;
constexpr u64 SS_REC_MASK = (1ull << 24) - 1;
constexpr u64 SS_SMALL_MAX = 16ull << 20;
__host__ __device__ inline u64 ss_key(u64 sec, u64 rec, u32 st) { return (sec << SS_SEC_SHIFT) | (rec << 4) | st; }
}  // namespace sidx
