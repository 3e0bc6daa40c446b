// sidx_stage.hpp -- the LDS-DMA tile staging the tile passes share (sidx_kernels.hip: FASTQ, FASTA,
// line, SAM; sidx_column.hip: column) and the LDS-only workgroup barrier that goes with it.
#pragma once
#include <hip/hip_runtime.h>

#include "sidx_common.hpp"
#include "sidx_device.hpp"

namespace sidx {

// Workgroup barrier for LDS hand-offs only.  __syncthreads() carries a workgroup-scope
// fence that waits vmcnt(0): on gfx950 (GFX9 counters) that drains every outstanding
// global load AND store of the wave -- the next tile's prefetch, the row stores, the
// look-back status stores -- at every barrier.  All intra-workgroup communication here is
// through LDS, so waiting for this wave's LDS operations is enough.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ====================================================================================
// LDS-DMA tile staging shared by the tile passes: a 256-thread workgroup stages one 16 KiB
// tile (+ the 16 bytes in front of it and a 1 KiB halo) into its LDS slot by buffer_load ...
// lds (1 KiB per wave-instruction, no VGPR destination), waits with vmcnt and classifies its
// own 64 bytes per thread into one '\n' mask word.
// ====================================================================================
constexpr int SNT = TILE / 64;                // threads per workgroup: one 64-byte '\n' mask word each
constexpr int SNW = SNT / 64;
static_assert(HALO % 256 == 0, "256-byte halo DMA pieces");
constexpr int SHPW = (HALO / 256 + SNW - 1) / SNW;  // halo pieces per wave (the last waves may have fewer)
constexpr int SSLOT = FRONT + TILE + HALO;    // LDS slot: [16 bytes before | tile | halo]
static_assert(SSLOT % 16 == 0, "16-byte aligned slots");
constexpr int SPER = TILE / 1024 / SNW;       // 1 KiB DMA wave-instructions per wave per tile
#ifndef SIDX_SNLCAP_DIV
#define SIDX_SNLCAP_DIV 16
#endif
constexpr int SNLCAP = TILE / SIDX_SNLCAP_DIV;  // '\n' positions kept (lines >= 16 B on average)
constexpr int SHW = HALO / 64;                // halo mask words (classified by the last wave)
static_assert(SHW <= 64, "halo words fit one wave");



constexpr int SHALO = HALO - FRONT;           // halo bytes past the tile read into a slot
typedef __attribute__((address_space(3))) uint8_t lds_u8;
// cache policy of the DMA: SIDX_DMA_NT bit 0 = the tile body non-temporal (read once), bit 1 =
// the 256-byte pieces (halo, front) too -- the halo is the next tile's first KiB, which the
// neighbouring workgroup on the same XCD reads, so it keeps the default policy.  Round 4, input
// in contiguous HBM, interleaved A/B on one box: k_fq_tiles 1.910 -> 1.874 ms with the body nt
// (bit 1 as well: slower); FASTA and line tiles take the nt body always (dma_piece16_nt)
#ifndef SIDX_DMA_NT
#define SIDX_DMA_NT 1
#endif
#if SIDX_DMA_NT & 1
#define SIDX_POL16 "nt "
#else
#define SIDX_POL16 ""
#endif
#if SIDX_DMA_NT & 2
#define SIDX_POL4 "nt "
#else
#define SIDX_POL4 ""
#endif
__device__ __forceinline__ void dma_piece16(u32 voff, u32 lds, __amdgpu_buffer_rsrc_t rs) {
  u32 keep;
  asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen " SIDX_POL16 "lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(lds), "s"(rs) : "memory");
}
// The tile body non-temporal: FASTA and line tiles (no halo read by a neighbour) -- A/B on one
// box, 10 GiB: k_fa_tiles 2.21 -> 2.15 ms, k_line_tiles 2.24 -> 2.06 ms; FASTQ unchanged, so it
// keeps the default policy (its halo is the next tile's first KiB, read through L2)
__device__ __forceinline__ void dma_piece16_nt(u32 voff, u32 lds, __amdgpu_buffer_rsrc_t rs) {
  u32 keep;
  asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen nt lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(lds), "s"(rs) : "memory");
}
__device__ __forceinline__ void dma_piece4(u32 voff, u32 lds, __amdgpu_buffer_rsrc_t rs) {
  u32 keep;
  lds = (u32)__builtin_amdgcn_readfirstlane((int)lds);  // uniform by construction (M0)
  asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dword %1, %3, 0 offen " SIDX_POL4 "lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(lds), "s"(rs) : "memory");
}
// P0: DMA of tile tn into the slot `dst` ([16 bytes in front | tile | halo], slot byte o = file
// byte tlo - FRONT + o).  Wave w stages the tile bytes [4096 w, 4096 (w + 1)) -- exactly the
// 64-byte words its own threads classify first -- as 4 pieces of 1 KiB (16 bytes per lane), so
// each wave starts on its masks after its own covering vmcnt, with no barrier: an LDS-DMA is
// ordered for the issuing wave's reads by its vmcnt alone (MI355X_MICROARCH.md, co-residence
// item 7), and other waves read those bytes only after a later barrier.  kFq: also the 16
// bytes in front (wave 0, 4 lanes of 4 bytes) and the halo (one 256-byte piece per wave), both
// read only after a barrier.  The buffer range [., min(., end)) is checked per dword: nothing
// past the slab's readable end is read (those dwords land as zeros).  For the file's first tile
// (no bytes in front) the base is the tile itself and the front piece's lanes fall out of range.
// The DMA is inline asm the compiler does not track: its waits are counted by hand, and no
// compiler-visible load is live across it in the loop.
// A wave's 4 KiB of the tile body as four pieces under one M0 (the instruction offset advances
// the global and the LDS address together) instead of one M0 save / set / restore per piece:
// A/B on one box (profiles/r04/ab_m0once.txt) k_fq_tiles 1.876 -> 1.855 ms, k_fa_tiles
// 2.134 -> 2.095 ms -- the tile passes issue a third of their instructions on the scalar unit.
// (Folding the FASTQ halo piece into the same statement measured the same: ab_halofold_fastq.txt.)
#ifndef SIDX_DMA_M0ONCE
#define SIDX_DMA_M0ONCE 1
#endif
template <bool kNt>
__device__ __forceinline__ void dma_body4(u32 voff, u32 lds, __amdgpu_buffer_rsrc_t rs) {
  u32 keep;
  if (kNt)
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen nt lds\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen offset:1024 nt lds\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen offset:2048 nt lds\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen offset:3072 nt lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds), "s"(rs) : "memory");
  else
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen lds\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen offset:1024 lds\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen offset:2048 lds\n\t"
                 "buffer_load_dwordx4 %1, %3, 0 offen offset:3072 lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds), "s"(rs) : "memory");
}
// stage_tile_at: the tile at `tile0` (its byte 0) with llen readable bytes from there on (at most
// TILE + SHALO); `shifted`: FRONT bytes are readable in front of it.  Only 32-bit values besides
// the base, all wave-uniform: what a claim loop keeps per tile (sidx_kernels.hip, ClaimBytes).
// plane: the lane number the predicates use (the claim loops pass an opaque copy, so that no
// predicate is kept in scalar registers from tile to tile).
template <bool kFq>
__device__ __forceinline__ void stage_tile_at(const uint8_t *tile0, u32 llen, bool shifted, u32 dst, int wid, int lane,
                                              int plane) {
  const u64 ba = (u64)tile0 - (shifted ? FRONT : 0);
  const u32 nrec = llen + (shifted ? FRONT : 0);
  const uint8_t *sbase = (const uint8_t *)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)ba)) |
                                           ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(ba >> 32)) << 32));
  const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)sbase, (short)0,
                                                    (int)__builtin_amdgcn_readfirstlane((int)nrec), 0x00020000);
  const u32 adj = shifted ? 0u : (u32)FRONT;  // unshifted: slot offsets are 16 bytes ahead of the base
  const u32 w0 = (u32)FRONT + (u32)(wid * SPER) * 1024u;
  if (SIDX_DMA_M0ONCE && SPER == 4) {
    dma_body4<!kFq || (SIDX_DMA_NT & 1)>(w0 + (u32)lane * 16u - adj, dst + w0, rs);
  } else {
#pragma unroll
    for (int i = 0; i < SPER; ++i) {
      if (kFq) dma_piece16(w0 + (u32)i * 1024u + (u32)lane * 16u - adj, dst + w0 + (u32)i * 1024u, rs);
      else dma_piece16_nt(w0 + (u32)i * 1024u + (u32)lane * 16u - adj, dst + w0 + (u32)i * 1024u, rs);
    }
  }
  if (!kFq) return;
  if (wid == 0 && plane < FRONT / 4) dma_piece4((u32)lane * 4u - adj, dst, rs);
  constexpr bool kAllPieces = SNW * SHPW == HALO / 256;  // every wave's pieces exist
#pragma unroll
  for (int h = 0; h < SHPW; ++h) {
    const int piece = wid * SHPW + h;
    const u32 h0 = (u32)(FRONT + TILE) + (u32)piece * 256u;
    if (kAllPieces || piece < HALO / 256) dma_piece4(h0 + (u32)lane * 4u - adj, dst + h0, rs);
  }
}
template <bool kFq>
__device__ __forceinline__ void stage_tile(const SlabParams &p, u64 tn, u32 dst, int wid, int lane) {
  const u64 tlo = tn * TILE;
  const u64 lim = (tlo + TILE + SHALO < p.end) ? tlo + TILE + SHALO : p.end;
  stage_tile_at<kFq>(p.data + tlo, (u32)(lim - tlo), tlo >= FRONT || p.front >= FRONT, dst, wid, lane, lane);
}

}  // namespace sidx
