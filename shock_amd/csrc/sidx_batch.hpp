// sidx_batch.hpp -- what the batch build's kernels (sidx_batch.hip) and its entry points
// (sidx_batch_api.cpp) share: the control words, the per-node result and the launch arguments.
#pragma once
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"

namespace sidx {

constexpr u64 BATCH_STEP = 1024;  // bytes a wave walks per step (64 lanes x 16 bytes)
constexpr u32 BATCH_PATH = 5;     // shockidx_batch_item::path of a node the batched walk indexed

enum BatchCtl : int {
  BC_INVALID = 0,   // a node outside the arena or misaligned: nothing else runs
  BC_NSINGLE = 1,   // nodes longer than the small limit (left to the single build)
  BC_TOTAL = 2,     // the table's extent in rows
  BC_GO = 3,        // 1: the list is valid and the table fits row_cap, so rows may be written
  BC_INTERNAL = 4,  // a device invariant was violated
  BC_NOK = 5,       // batched nodes whose status is OK
  BC_NWORDS = 8
};

// One node's result; the layout of shockidx_batch_item (include/shockidx.h)
struct BatchItem {
  u64 count, row_off;
  int format, status;
  u32 term_code, path;
  u64 err_pos, err_len;
};
static_assert(sizeof(BatchItem) == 48, "copied out as shockidx_batch_item");

// a node left to the single build, as the classify kernel reports it
struct BatchSingle {
  u64 node;
  i64 pos, len;
};

struct BatchArgs {
  const uint8_t *data;  // the arena (16-byte aligned)
  u64 data_len;
  const i64 *nodes;     // {pos, len} per node
  u64 K;
  u64 small;            // the small-node limit in bytes (0: every node is a single)
  int fmt;              // the format given for all nodes (F_*), F_NONE: detect per node
  int verify;           // check every finished table (SHOCKIDX_VERIFY)
  int *nfmt;            // per node: its format
  u64 *nat;             // per node: the rows it has when no record ends it early
  u64 *base;            // per node: its first row in the table (exclusive scan of nat)
  u64 *key;             // per node: min (record << 4 | status) over its terminating records, ~0: none
  u64 *ctl;             // BatchCtl words
  BatchSingle *singles;
  u64 *rows;
  u64 row_cap;
  BatchItem *items;
};

}  // namespace sidx
