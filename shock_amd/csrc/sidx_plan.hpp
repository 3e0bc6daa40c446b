// sidx_plan.hpp -- control words and launch geometry shared by the download-plan kernels
// (sidx_plan.hip) and their entry point (sidx_plan_api.cpp).
#pragma once
namespace sidx {
// control words of one plan, kept on the device; the host reads them at its waits
enum PlanCtl : int {
  PC_ERRKEY = 0,  // min over invalid level-2 segments of (part << 32 | record-in-request), ~0: none
  PC_N1 = 1,      // level-1 records (CHUNK_RANGE: the level-2 segments)
  PC_V2 = 2,      // rows level 2 visits
  PC_NSEC = 3,    // sections of the plan
  PC_SIZE = 4,    // Go's size: the sections' lengths summed mod 2^64
  PC_NWORDS = 8
};
constexpr unsigned PLAN_THREADS = 256;  // visits per workgroup of the flag and emit passes
}  // namespace sidx
