// sidx_subset.hpp -- status codes shared by the subset kernels and the C ABI.
#pragma once
namespace sidx {
// per-id outcome, in the order subset.go:201-223 checks them
enum SubStatus : unsigned {
  SUB_OK = 0,
  SUB_SYNTAX = 1,  // strconv.Atoi: parsing "...": invalid syntax
  SUB_RANGE = 2,   // strconv.Atoi: parsing "...": value out of range
  SUB_SORT = 3,    // Subset indices must be numerically sorted and non-redundant, ...
  SUB_EXIST = 4,   // Subset index: %d does not exist in parent index file.
  SUB_READ = 5,    // Subset index could not read parent index file for part: %d
};
// control words of one subset build, kept on the device (the host reads them once, at the end)
enum SubCtl : int {
  SC_FIRSTBAD = 0,  // min over failing ids of (rank << 3 | SubStatus), ~0: none
  SC_SIZE = 1,      // oSize
  SC_K = 2,         // non-blank ids
  SC_KE = 3,        // ids accepted before the first failing one
  SC_NSTART = 4,    // runs among them
  SC_FLAGS = 5,     // 1: rows_cap < Ke, 2: runs_cap < runs, 4: out_cap < the gathered bytes
  SC_TOTAL = 6,     // gathered bytes
  SC_NWORDS = 8,
  // oSize is summed into SC_SLOTS slots past the control words, one per group of workgroups
  // (6,000 workgroups adding into one word at C4 took most of k_sub_runs' 78 us); the host adds them
  SC_SLOTS = 64,
  SC_ALLWORDS = SC_NWORDS + SC_SLOTS
};
// ---- the subset walk in slabs (shockidx_subset_slab_device) ---------------------------------
// subset.go:168-176's loop state as one slab call leaves it: a call reads half[which] and writes
// the other half, then flips `which`, so a call that returns early leaves the carry as it was.
struct SubCarryHalf {
  unsigned long long next_off;  // offset of the first id line not yet consumed
  long long prev_id;            // prev_int
  unsigned long long prev_off, prev_len;  // prevOffset, prevLength
  unsigned long long co_off;    // coOffset of the open run (coLength = prev_off + prev_len - co_off)
  unsigned long long count, nruns, size;  // oCount, coCount, oSize
};
struct SubCarry {
  unsigned long long magic;  // SUBCARRY_MAGIC once the first slab has initialised it
  unsigned state;            // SubWalkState
  unsigned which;
  SubCarryHalf half[2];
};
constexpr unsigned long long SUBCARRY_MAGIC = 0x5355425743415259ull;
enum SubWalkState : unsigned { SW_WALK = 1, SW_DONE = 2, SW_ERROR = 3 };
// control words of one slab call (the first SC_NWORDS as SubCtl's: k_sub_compact writes SC_K)
enum SubSlabCtl : int {
  SL_FIRSTBAD = SC_FIRSTBAD,  // min over failing ids of (rank << 3 | SubStatus), ~0: none
  SL_SIZE = SC_SIZE,          // the lengths of the rows this call consumed
  SL_K = SC_K,
  SL_KE = SC_KE,              // ids consumed by this call
  SL_NCLOSED = 4,             // runs closed by them
  SL_FLAGS = 5,               // 1: the carry does not allow this call
  SL_FIRSTOUT = 6,            // min rank of an accepted id whose row is outside the window, ~0: none
  SL_STOP = 7,
  SL_NEXT_OFF = 8,
  SL_NEXT_ID = 9,
  SL_FINAL = 10,              // 1: the final run is written (subset.go:285-291)
  SL_CODE = 11,               // SubStatus of the failing id, 0: none
  SL_ERR_V = 12,
  SL_ERR_PREV = 13,
  SL_ERR_OFF = 14,            // the failing line, relative to the slab's first byte, and its length
  SL_ERR_LEN = 15,
  SL_COUNT = 16,              // the running totals after this call
  SL_NRUNS = 17,
  SL_TOTSIZE = 18,
  SL_TAIL = 19,               // the owned line that does not close inside the window (relative), ~0: none
  SL_START = 20,              // lines starting at or after this (relative) are not yet consumed
  SL_BASE_LS = 21,            // the slab's first byte starts a line
  SL_NEWCO = 22,              // coOffset of the run the last run start of this call opened
  SL_WORDS = 24
};
// one slab call's arguments and workspace, as its kernels take them (by value)
struct SubSlabArgs {
  const unsigned char *text;  // the slab's first byte (16-byte aligned); [text - front, text + end) is readable
  unsigned long long n, end, front, base, ids_size;
  int is_first, is_last, want_runs;
  const unsigned long long *parent;  // rows [prow0, prow0 + prows) of the parent index
  unsigned long long prow0, prows, parent_count;
  long long ilength;
  SubCarry *carry;
  unsigned long long *rows, rows_cap, *runs, runs_cap;
  unsigned long long m;  // '\n's in [text, text + end)
  // workspace: ends[m]; per line keep, val, st, rank (startf = keep and runid = rank after the compaction); per id cval, cst, cline
  const unsigned long long *ends;
  unsigned *keep;
  long long *val;
  unsigned *st;
  unsigned long long *rank;
  long long *cval;
  unsigned *cst;
  unsigned long long *cline, *ctl;
};
#ifndef SIDX_GB_BLOCK
#define SIDX_GB_BLOCK 32768
#endif
constexpr unsigned GATHER_BLOCK = SIDX_GB_BLOCK;  // output bytes per k_gather workgroup (the plan's unit)
}  // namespace sidx
