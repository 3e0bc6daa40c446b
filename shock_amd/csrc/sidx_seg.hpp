// sidx_seg.hpp -- the wave walk over one segment (a section of the stream, a node of the batch
// build), 16 bytes per lane and 1 KiB per step: what a lane has to know about the bytes before
// its own, carried from lane to lane and from step to step.  Shared by sidx_stream.hip and
// sidx_batch.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"
#include "sidx_device.hpp"

namespace sidx {

// the last set byte of a lane's mask in its 1 KiB step, position in the step + 1 (0: none)
__device__ __forceinline__ u32 ss_last_in_step(u32 m, int lane) {
  return m ? 16u * (u32)lane + 32u - (u32)__builtin_clz(m) : 0u;
}
// the wave's exclusive maximum of v (0 in lane 0) and its maximum over all lanes
__device__ __forceinline__ u32 ss_excl_max(u32 v, int lane, u32 &all) {
  const u32 inc = wave_scan_max(v);
  all = (u32)__shfl((int)inc, 63, 64);
  const u32 p = (u32)__shfl_up((int)inc, 1, 64);
  return lane ? p : 0u;
}

// The boundary '>' bits of the lane's 16 bytes at a (bnd_bits of sidx_filter.hip for a 16-bit word);
// cnl / cgt: the section's last '\n' / '>' before this 1 KiB step (position + 1, 0: none), carried on
// to the next step.
__device__ __forceinline__ u32 ss_fa_bnd(u32 mnl, u32 mgt, u64 a, u64 b0, int lane, u64 &cnl, u64 &cgt) {
  u32 tnl, tgt;
  const u32 pnl = ss_excl_max(ss_last_in_step(mnl, lane), lane, tnl);
  const u32 pgt = ss_excl_max(ss_last_in_step(mgt, lane), lane, tgt);
  const u64 lnl = pnl ? b0 + pnl : cnl, lgt = pgt ? b0 + pgt : cgt;  // before the lane's bytes
  u32 out = 0;
  for (u32 m = mgt; m; m &= m - 1) {
    const u32 i = (u32)__builtin_ctz(m), below = (1u << i) - 1u;
    const u64 ln = (mnl & below) ? a + 32 - (u64)__builtin_clz(mnl & below) : lnl;
    const u64 lg = (mgt & below) ? a + 32 - (u64)__builtin_clz(mgt & below) : lgt;
    if (ln > lg) out |= 1u << i;
  }
  if (tnl) cnl = b0 + tnl;
  if (tgt) cgt = b0 + tgt;
  return out;
}

}  // namespace sidx
