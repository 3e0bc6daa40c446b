// sidx_kernels.hip -- gfx950 kernels of the MI355X record indexer: every kernel of an index
// build (format detection, the slab exchange and the table check are in sidx_control.hip).
//
//   k_fq_tiles     FASTQ tile pass: LDS-DMA staged 16 KiB tiles, '\n' masks, the record phase
//                  read off the tile, records certified from LDS into a provisional row table
//   k_fa_tiles     FASTA tile pass (the FastaMonoid boundaries, pieces validated from LDS)
//   k_line_tiles   line tile pass ('\n' positions per tile); k_sam_tiles the SAM one (terminator lines)
//   k_scan_excl<M> device-wide exclusive scan of the per-tile aggregates (decoupled look-back)
//   k_*_place      final 16-byte rows at their global record numbers; k_fixup / k_fa_fixup
//                  re-validate from global memory what a tile could not settle
//   k_tile_agg<F> + k_index1<F>  the two-pass build (SAM slabs, re-runs)
//   k_finalize   folds the slab's terminal state + first-bad key into a DevResult
//
// Reference semantics restated (paths relative to /root/reference/shock-server/):
//   record driver  node/file/index/record.go:34-90     line driver node/file/index/line.go:33-85
//   FASTQ          node/file/format/fastq/fastq.go:134-213
//   FASTA          node/file/format/fasta/fasta.go:93-140
//   SAM            node/file/format/sam/sam.go:83-98
//   line           node/file/format/line/line.go:37-45
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <atomic>

#include "sidx_claim.hpp"
#include "sidx_common.hpp"
#include "sidx_device.hpp"
#include "sidx_launch.hpp"
#include "sidx_stage.hpp"
#include "sidx_validate.hpp"

namespace sidx {

// Diagnostics (phase timing, ablation knobs) exist only in the SIDX_DIAG=1 variant build
// (make variant V=diag VFLAGS=-DSIDX_DIAG=1): runtime-uniform flags in the production
// kernels would make the compiler clone the hot loops once per flag combination.
#ifndef SIDX_DIAG
#define SIDX_DIAG 0
#endif
__device__ __forceinline__ u32 dbg(const SlabParams &p) { return SIDX_DIAG ? p.debug : 0u; }
__device__ __forceinline__ u64 *tmg(const SlabParams &p) { return SIDX_DIAG ? p.timing : nullptr; }

// ====================================================================================
// Format traits
// ====================================================================================
template <int F> struct Traits;
template <> struct Traits<F_FASTQ> { typedef CountMonoid M; static constexpr bool kX = false; static constexpr u32 xc = 0; };
template <> struct Traits<F_LINE>  { typedef CountMonoid M; static constexpr bool kX = false; static constexpr u32 xc = 0; };
template <> struct Traits<F_FASTA> { typedef FastaMonoid M; static constexpr bool kX = true; static constexpr u32 xc = '>'; };
template <> struct Traits<F_SAM>   { typedef SamMonoid M;   static constexpr bool kX = true; static constexpr u32 xc = '@'; };

// FASTQ / LINE keep the tile's '\n' positions (tile-relative u16) in LDS: a record is then
// 4 (FASTQ) or 1 (line) consecutive entries and needs no search.  Tiles with more newlines
// than NLCAP (lines shorter than 8 bytes on average) use the region walk instead.
constexpr int NLCAP = TILE / 8;
constexpr int NLHALO = 4;  // newlines past the tile end kept in nlpos (one FASTQ record)
template <int F> constexpr bool kNlArray() { return F == F_FASTQ || F == F_LINE; }

template <int F, int NLC = NLCAP>
struct __align__(16) Smem {
  uint8_t raw[FRONT + TILE + HALO];  // raw[0] = byte tlo - FRONT
  u64 mnl[(TILE + HALO) / 64];
  u64 mx[Traits<F>::kX ? (TILE + HALO) / 64 : 1];
  uint16_t nlpos[kNlArray<F>() ? NLC : 1];
  u64 wtot[NWAVES];
  u64 tile_in;
  u64 badkey;
  u64 defer_s[MAX_DEFER];
  u64 defer_k[MAX_DEFER];
  u64 defer_aux[MAX_DEFER];
  u32 ndefer;
  u32 nh;  // newlines past the tile end in nlpos[T..T+nh)
  // FASTA: nextx[w] = tile-relative position of the first '>' in mask words >= w of
  // tile + halo (0xFFFF: none), so a lane finds the next '>' without walking the words
  uint16_t nextx[F == F_FASTA ? (TILE + HALO) / 64 + 1 : 1];
};

// any set bit of the 128-bit region mask (w0 | w1 << 64) in [lo, hi)
__device__ __forceinline__ bool any128(u64 w0, u64 w1, u32 lo, u32 hi) {
  if (lo >= hi) return false;
  u64 m0 = 0, m1 = 0;
  if (lo < 64) m0 = (~0ull << lo) & (hi >= 64 ? ~0ull : lowmask(hi));
  if (hi > 64) m1 = (lo > 64 ? (~0ull << (lo - 64)) : ~0ull) & lowmask(hi - 64);
  return (w0 & m0) || (w1 & m1);
}

// One record for the emission / deferred paths: validate and write its row or bad key.
struct Bad {
  u64 key = KEY_NONE, pos = 0, len = 0;
};

// out-of-line instances for the rare / cold call sites (keeps the hot loop small)
template <int F, class A>
__device__ __noinline__ u32 run_record_cold(A &a, u64 s, u64 aux, u64 &len, u64 &epos, u64 &elen) {
  return run_record<F>(a, s, aux, len, epos, elen);
}

__device__ __forceinline__ void put_row(const SlabParams &p, u64 k, u64 s, u64 len) {
  const u64 i = k - p.row_base;
  if (k >= p.row_base && i < p.row_cap) {
    ulonglong2 v;
    v.x = p.base + s;
    v.y = len;
    reinterpret_cast<ulonglong2 *>(p.rows)[i] = v;
  }
}

__device__ __forceinline__ void note_bad(Bad &b, u64 k, u32 tile, u32 st, u64 pos, u64 len) {
  const u64 key = bad_key(k, tile, st);
  if (key < b.key) { b.key = key; b.pos = pos; b.len = len; }
}

template <int F>
__device__ __forceinline__ void defer_record(const SlabParams &p, Smem<F> *sm, u64 s, u64 k, u64 aux) {
  const u32 slot = atomicAdd(&sm->ndefer, 1u);
  if (slot < MAX_DEFER) {
    sm->defer_s[slot] = s;
    sm->defer_k[slot] = k;
    sm->defer_aux[slot] = aux;
  } else {
    atomicAdd(&p.counters[1], 1u);  // never silently dropped: finalize flags an error
  }
}

template <int F, class A>
__device__ __forceinline__ void finish_record(const SlabParams &p, A &a, u32 tile, u64 s, u64 k,
                                              u64 aux, Bad &bad, Smem<F> *sm) {
  u64 len = 0, epos = 0, elen = 0;
  const u32 st = run_record<F>(a, s, aux, len, epos, elen);
  if (st == ST_OK) put_row(p, k, s, len);
  else if (st == ST_DEFER) defer_record<F>(p, sm, s, k, aux);
  else note_bad(bad, k, tile, st, p.base + epos, elen);
}

__device__ __forceinline__ bool ascii_nonspace(u32 c) { return c < 0x80 && !ascii_space(c); }

template <class A>
__device__ __forceinline__ u64 trimmed_len(A &a, u64 lo, u64 hi) {
  u64 tl, th;
  trim_space(a, lo, hi, tl, th);
  return th - tl;
}

// fastq.go:134-213 for a group whose four line ends e0..e3 are known (tile-relative, all
// staged in LDS): no searching, just the checks in Go's order.  A plus line that carries an
// ID (:195-199) is reported through needcmp/ilo/plo1/clen and compared by the whole wave;
// the length check (:202-207) that follows it comes back in lenbad.  Blank id lines take
// the general validator (ST_SLOW).
__device__ __forceinline__ u32 fq_known(const LaneAcc &a, u32 s, u32 e0, u32 e1, u32 e2, u32 e3, u32 &len,
                                        bool &needcmp, u32 &ilo, u32 &plo1, u32 &clen, bool &lenbad) {
  const uint8_t *r = a.raw + FRONT;
  if (e0 == s) return ST_SLOW;  // blank: skip-loop semantics (general validator)
  if (r[s] != '@') return ST_FQ_NOAT;
  if (e0 - s == 1) return ST_FQ_NOID;
  if (e1 == e0 + 1) return ST_FQ_EMPTYSEQ;
  if (r[e1 + 1] != '+') return ST_FQ_NOPLUS;
  const u64 tlo = a.tlo;
  if (e2 - e1 != 2) {
    u64 plo, phi;
    trim_space(a, tlo + e1 + 1, tlo + e2 + 1, plo, phi);
    if (phi - plo > 1) {
      u64 il, ih;
      trim_space(a, tlo + s + 1, tlo + e0 + 1, il, ih);
      if (ih - il != phi - plo - 1) return ST_FQ_IDMISMATCH;
      needcmp = ih > il;
      ilo = (u32)(il - tlo); plo1 = (u32)(plo + 1 - tlo); clen = (u32)(ih - il);
    }
  }
  u32 sl, ql;
  if (ascii_nonspace(r[e0 + 1]) && ascii_nonspace(r[e1 - 1])) sl = e1 - e0 - 1;
  else sl = (u32)trimmed_len(a, tlo + e0 + 1, tlo + e1 + 1);
  if (e3 > e2 + 1 && ascii_nonspace(r[e2 + 1]) && ascii_nonspace(r[e3 - 1])) ql = e3 - e2 - 1;
  else ql = (u32)trimmed_len(a, tlo + e2 + 1, tlo + e3 + 1);
  lenbad = sl != ql;
  len = e3 + 1 - s;
  return ST_OK;
}

// ====================================================================================
// Look-back (wave 0).  Status words are read and written through global (address space
// 1) agent-scope atomics only -- global_load/store ... sc1, never flat (guide §6 G16).
// ====================================================================================
typedef __attribute__((address_space(1))) u64 gu64;

__device__ __forceinline__ u64 st_load(gu64 *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_store(gu64 *p, u64 v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u32 wflag(u64 w, u32 epoch) {
  return (((u32)(w >> EPOCH_SHIFT)) & EPOCH_MASK) == epoch ? (u32)(w >> 62) : 0u;
}


// ====================================================================================
// Two-pass build (k_index1<F>): one tile per workgroup, 16 B/lane buffer loads staged into
// LDS with the tile's class masks, incoming state from the scanned tile aggregates.
// ====================================================================================
__device__ __forceinline__ uint4 to_u4(__attribute__((ext_vector_type(4))) unsigned int x) {
  return make_uint4(x[0], x[1], x[2], x[3]);
}
// zero the bytes of v at index >= nb (0 < nb < 16)
__device__ __forceinline__ uint4 keep_bytes(uint4 v, u32 nb) {
  const u32 k0 = nb >= 4 ? ~0u : ((1u << (8 * nb)) - 1u);
  const u32 k1 = nb >= 8 ? ~0u : (nb <= 4 ? 0u : ((1u << (8 * (nb - 4))) - 1u));
  const u32 k2 = nb >= 12 ? ~0u : (nb <= 8 ? 0u : ((1u << (8 * (nb - 8))) - 1u));
  const u32 k3 = nb <= 12 ? 0u : ((1u << (8 * (nb - 12))) - 1u);
  return make_uint4(v.x & k0, v.y & k1, v.z & k2, v.w & k3);
}

// Tile loads through a buffer descriptor covering exactly [tlo, lhi).  The range check works
// on whole dwords: a dword that is not entirely inside returns 0, so only the last, partial
// dword of a slab needs bytes of its own (trim_tile).  The descriptor is built from
// wave-uniform values made explicitly scalar: a descriptor the compiler cannot prove uniform
// becomes a waterfall loop that waits for every load.  No loaded value is touched here (the
// loads stay in flight until stage_tile).
__device__ __forceinline__ u32 tile_llen(const SlabParams &p, u64 tile) {
  const u64 tlo = tile * TILE;
  const u64 lhi = (tlo + TILE + HALO < p.end) ? tlo + TILE + HALO : p.end;
  return (u32)(lhi - tlo);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const SlabParams &p, u64 tile, u32 &llen) {
  const u64 ba = (u64)(p.data + tile * TILE);
  llen = (u32)__builtin_amdgcn_readfirstlane((int)tile_llen(p, tile));
  const uint8_t *sbase = (const uint8_t *)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)ba)) |
                                           ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(ba >> 32)) << 32));
  return __builtin_amdgcn_make_buffer_rsrc((void *)sbase, (short)0, (int)llen, 0x00020000);
}
__device__ __forceinline__ void load_tile_buf(const SlabParams &p, u64 tile, int tid, uint4 (&v)[CPT + 1]) {
  const u64 tlo = tile * TILE;
  u32 llen;
  const auto rs = tile_rsrc(p, tile, llen);
  // one VGPR offset (this thread's chunk) + a constant scalar offset per chunk: no per-chunk
  // address registers to keep live (or spill) across the loop
  const int voff = tid * CHUNK;
#pragma unroll
  for (int k = 0; k < CPT; ++k)
    v[k] = to_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, voff, k * NTHREADS * CHUNK, 0));
  if (tid < HALO_CHUNKS) {
    v[CPT] = to_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, voff, CPT * NTHREADS * CHUNK, 0));
  } else if (tid == HALO_CHUNKS) {
    v[CPT] = (tlo >= FRONT || p.front >= FRONT) ? load16(p.data + tlo - FRONT) : make_uint4(0, 0, 0, 0);
  }
}
// the readable end falls inside a dword (a slab's last tile only): fetch its bytes
__device__ __forceinline__ u32 tail_dword(const __amdgpu_buffer_rsrc_t rs, u32 llen) {
  const u32 d = llen & ~3u;
  u32 w = 0;
  for (u32 i = 0; i < (llen & 3u); ++i) w |= (u32)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)(d + i), 0, 0) << (8 * i);
  return w;
}
__device__ __forceinline__ void patch_tail(uint4 &x, u32 off, u32 llen, u32 w) {
  const u32 q = ((llen & ~3u) - off) >> 2;  // dword of the chunk holding the end
  if (q == 0) x.x = w; else if (q == 1) x.y = w; else if (q == 2) x.z = w; else x.w = w;
}
__device__ __forceinline__ void trim_tile(const SlabParams &p, u64 tile, int tid, uint4 (&v)[CPT + 1]) {
  if (tile_llen(p, tile) >= (u32)(TILE + HALO) || (tile_llen(p, tile) & 3u) == 0) return;  // uniform
  u32 llen;
  const auto rs = tile_rsrc(p, tile, llen);
  const u32 w = tail_dword(rs, llen);
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const u32 off = (u32)(k * NTHREADS + tid) * CHUNK;
    if (off < llen && off + CHUNK > llen) patch_tail(v[k], off, llen, w);
  }
  if (tid < HALO_CHUNKS) {
    const u32 off = (u32)(CPT * NTHREADS + tid) * CHUNK;
    if (off < llen && off + CHUNK > llen) patch_tail(v[CPT], off, llen, w);
  }
}

__device__ __forceinline__ u64 stamp() {
  u64 t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

template <int F>
__device__ __forceinline__ void process_tile(const SlabParams &p, gu64 *status, u32 tile, Smem<F> &sm,
                                             int tid, int lane, int wid, u64 *ts) {
  typedef typename Traits<F>::M M;
  const u64 tlo = (u64)tile * TILE;
  const u64 thi = (tlo + TILE < p.n) ? tlo + TILE : p.n;
  const u32 tlen = (u32)(thi - tlo);

  // ---- region (128 contiguous bytes per thread) aggregates + ordered block scan --------
  const u32 rlo = (u32)tid * REGION;
  const u32 len0 = tlen > rlo ? (tlen - rlo >= 64 ? 64u : tlen - rlo) : 0u;
  const u32 len1 = tlen > rlo + 64 ? (tlen - rlo - 64 >= 64 ? 64u : tlen - rlo - 64) : 0u;
  // only bytes the slab owns: the halo past a slab's end belongs to the next slab's records
  const u64 nl0 = sm.mnl[2 * tid] & lowmask(len0), nl1 = sm.mnl[2 * tid + 1] & lowmask(len1);
  const u64 x0 = Traits<F>::kX ? sm.mx[2 * tid] & lowmask(len0) : 0;
  const u64 x1 = Traits<F>::kX ? sm.mx[2 * tid + 1] & lowmask(len1) : 0;
  const u64 ragg = M::combine(M::seg(nl0, x0, len0), M::seg(nl1, x1, len1));
  const u64 incl = wave_incl_scan<M>(ragg, lane);
  if (lane == 63) sm.wtot[wid] = incl;
  u64 lexcl = __shfl_up(incl, 1, 64);
  if (lane == 0) lexcl = M::identity();
  lds_barrier();
  u64 wpre = M::identity();
  for (int w = 0; w < wid; ++w) wpre = M::combine(wpre, sm.wtot[w]);
  const u64 texcl = M::combine(wpre, lexcl);
  u64 tagg = M::identity();
  for (int w = 0; w < NWAVES; ++w) tagg = M::combine(tagg, sm.wtot[w]);
  if (ts) ts[1] = stamp();

  // ---- incoming state: the exclusive prefix of the tile aggregates (scanned beforehand) ----
  if (wid == 0 && lane == 0) sm.tile_in = M::apply(p.state_in, p.tile_excl[tile]);
  // nlpos[0..T) = the tile's '\n' positions in order; nlpos[T..T+nh) = the first NLHALO
  // newlines past the tile end (line ends of the records that cross it), found by the last
  // wave
  const bool use_arr = kNlArray<F>() && tagg + NLHALO <= (u64)NLCAP;
  if (kNlArray<F>() && use_arr) {
    u32 o = (u32)texcl;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u64 m = h ? nl1 : nl0;
      while (m) {
        sm.nlpos[o++] = (uint16_t)(rlo + 64 * h + ctz64(m));
        m &= m - 1;
      }
    }
    if (wid == NWAVES - 1) {
      const u32 lhi_rel = (u32)(((tlo + TILE + HALO < p.end) ? tlo + TILE + HALO : p.end) - tlo);
      const u32 wb = tlen >> 6;  // first mask word holding bytes past the tile end
      u32 c = 0;
      u64 m = 0;
      const u32 wd = wb + (u32)lane;
      if (wd * 64 < lhi_rel) {
        m = sm.mnl[wd];
        if (wd == wb) m &= ~lowmask(tlen & 63);
        if (wd * 64 + 64 > lhi_rel) m &= lowmask(lhi_rel - wd * 64);
        c = popc64(m);
      }
      u32 pre = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(pre, d, 64);
        if (lane >= d) pre += y;
      }
      u32 o2 = pre - c;
      while (m && o2 < (u32)NLHALO) {
        sm.nlpos[(u32)tagg + o2] = (uint16_t)(wd * 64 + ctz64(m));
        ++o2;
        m &= m - 1;
      }
      if (lane == 63) sm.nh = pre < (u32)NLHALO ? pre : (u32)NLHALO;
    }
  }
  if (tid == 0) { sm.ndefer = 0; sm.badkey = KEY_NONE; }
  if (F == F_FASTA && wid == NWAVES - 1) {  // suffix min over the '>' mask words, 64 per step
    constexpr u32 NW = (TILE + HALO) / 64;
    u32 carry = 0xFFFFu;
    if (lane == 0) sm.nextx[NW] = 0xFFFFu;
    for (int b = (int)((NW - 1) / 64) * 64; b >= 0; b -= 64) {
      const u32 w = (u32)b + (u32)lane;
      u32 x = 0xFFFFu;
      if (w < NW) {
        const u64 m = sm.mx[w];
        if (m) x = w * 64 + ctz64(m);
      }
      // suffix min within the wave (lane i: min over lanes >= i), then the carry from above
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u32 y = (u32)__shfl_down((int)x, d, 64);
        if (lane + d < 64 && y < x) x = y;
      }
      if (carry < x) x = carry;
      if (w < NW) sm.nextx[w] = (uint16_t)x;
      carry = (u32)__shfl((int)x, 0, 64);
    }
  }
  if (ts) ts[2] = stamp();
  lds_barrier();
  if (ts) ts[3] = stamp();
  if (dbg(p) & 1) return;  // ablation: scan only
  const u64 tile_state = sm.tile_in;
  const u64 tin = M::apply(tile_state, texcl);  // state before this thread's region

  // ---- emission: records owned by this tile ---------------------------------------------
  LaneAcc acc;
  acc.raw = sm.raw; acc.mnl = sm.mnl; acc.mx = sm.mx;
  if (F == F_FASTA) acc.nextx = sm.nextx;
  acc.tlo = tlo; acc.lhi = (tlo + TILE + HALO < p.end) ? tlo + TILE + HALO : p.end;
  acc.end = p.end; acc.eof = p.eof; acc.dbg = dbg(p); acc.front = p.front;
  Bad bad;

  if (kNlArray<F>() && use_arr) {
    const u32 T = (u32)tagg;  // newlines in the tile; nlpos[0..T)
    const u64 j0 = tile_state;  // rank of the tile's first '\n'
    if (F == F_FASTQ) {
      // groups start after '\n' #j with j % 4 == 3 (and at file offset 0); a group whose four
      // line ends are in nlpos (tile + halo) is checked by fq_known, the rest (blank lines,
      // EOF, records longer than the halo) by the general validator
      const u32 TT = T + sm.nh;
      const u32 i0 = (u32)((3 - (j0 & 3)) & 3);
      const u32 ng = i0 < T ? (T - i0 + 3) / 4 : 0;
      for (u32 qb = (u32)wid * 64; qb < ng + 1; qb += NTHREADS) {  // wave-uniform trip count
        const u32 q = qb + (u32)lane;
        bool act = q < ng + 1;
        u32 s = 0, i = 0;
        u64 g = 0;
        if (act && q == ng) {  // the file-start group, owned by tile 0
          act = p.file_start && tile == 0;
        } else if (act) {
          const u32 d = i0 + 4 * q;
          s = sm.nlpos[d] + 1u; g = (j0 + d + 1) >> 2; i = d + 1;
        }
        if (dbg(p) & 32) act = false;
        u32 st = ST_SLOW, len = 0, ilo = 0, plo1 = 0, clen = 0;
        bool needcmp = false, lenbad = false;
        if (act && i + 3 < TT)
          st = fq_known(acc, s, sm.nlpos[i], sm.nlpos[i + 1], sm.nlpos[i + 2], sm.nlpos[i + 3], len, needcmp,
                        ilo, plo1, clen, lenbad);
        // fastq.go:195-199 ID compare, wave-cooperative: one record at a time, 64 bytes per step
        u64 mc = __ballot(act && st == ST_OK && needcmp);
        bool idmis = false;
        while (mc) {
          const int L = (int)ctz64(mc);
          mc &= mc - 1;
          const u32 a = (u32)__shfl((int)ilo, L, 64), b = (u32)__shfl((int)plo1, L, 64);
          const u32 n = (u32)__shfl((int)clen, L, 64);
          bool ne = false;
          for (u32 k = (u32)lane; k < n; k += 64) ne |= sm.raw[FRONT + a + k] != sm.raw[FRONT + b + k];
          const bool any = __ballot(ne) != 0;
          if (lane == L) idmis = any;
        }
        if (st == ST_OK && needcmp && idmis) st = ST_FQ_IDMISMATCH;
        else if (st == ST_OK && lenbad) st = ST_FQ_LENMISMATCH;
        if (!act) continue;
        u64 glen = len, epos = 0, elen = 0;
        if (st == ST_SLOW) st = run_record_cold<F>(acc, tlo + s, 0, glen, epos, elen);
        if (st == ST_OK) { if (!(dbg(p) & 16)) put_row(p, g, tlo + s, glen); }
        else if (st == ST_DEFER) defer_record<F>(p, &sm, tlo + s, g, 0);
        else note_bad(bad, g, tile, st, 0, 0);
      }
    } else {  // F_LINE: one row per line, row j+1 starts after '\n' #j
      for (u32 q = tid; q < T + 1; q += NTHREADS) {
        u64 s, k;
        u32 i;
        if (q == T) {
          if (!(p.file_start && tile == 0)) continue;
          s = 0; k = 0; i = 0;
        } else {
          s = sm.nlpos[q] + 1u; k = j0 + q + 1; i = q + 1;
        }
        if (i < T + sm.nh) put_row(p, k, tlo + s, (u64)sm.nlpos[i] + 1 - s);
        else finish_record<F>(p, acc, tile, tlo + s, k, 0, bad, &sm);
      }
    }
  } else {
    if (p.file_start && tile == 0 && tid == 0) {  // record 0 starts at file offset 0
      u64 aux = 0;
      if (F == F_FASTA) aux = (p.end > 0 && acc.byte(0) == '>') ? 1 : 0;
      finish_record<F>(p, acc, tile, 0, 0, aux, bad, &sm);
    }
    if (F == F_FASTQ || F == F_LINE) {
      u64 j = tin;  // global '\n' rank of the next newline
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        u64 m = h ? nl1 : nl0;
        while (m) {
          const u64 q = tlo + rlo + 64 * h + ctz64(m);
          m &= m - 1;
          if (F == F_LINE) finish_record<F>(p, acc, tile, q + 1, j + 1, 0, bad, &sm);
          else if ((j & 3) == 3) finish_record<F>(p, acc, tile, q + 1, (j + 1) >> 2, 0, bad, &sm);
          ++j;
        }
      }
    } else if (F == F_FASTA) {
      u64 cnt = tin >> 1;
      u32 armed = tin & 1;
      u32 pos = 0;  // region-relative
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        u64 m = h ? x1 : x0;
        while (m) {
          const u32 g = 64 * h + ctz64(m);
          m &= m - 1;
          if (any128(nl0, nl1, pos, g)) armed = 1;  // '\n' since the previous '>'
          if (armed) {
            ++cnt;
            const u64 b = tlo + rlo + g;
            finish_record<F>(p, acc, tile, b, cnt, b + 1, bad, &sm);
          }
          armed = 0;
          pos = g + 1;
        }
      }
    } else {  // F_SAM
      u64 cnt = tin >> 2;
      const u32 st0 = tin & 3;
      bool first = true;
      u64 prev = 0;  // tile-relative position of the previous '\n' in this region
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        u64 m = h ? nl1 : nl0;
        while (m) {
          const u64 q = rlo + 64 * h + ctz64(m);
          m &= m - 1;
          bool term;
          if (first && st0 != 0) {
            term = (st0 == 1);
          } else {
            const u64 ls = first ? (u64)rlo : prev + 1;
            term = (ls < q) && acc.byte(tlo + ls) != '@';
          }
          first = false;
          prev = q;
          if (term) {
            ++cnt;
            finish_record<F>(p, acc, tile, tlo + q + 1, cnt, 0, bad, &sm);
          }
        }
      }
    }
  }
  if (ts) ts[4] = stamp();
  lds_barrier();
  if (ts) ts[5] = stamp();

  // ---- deferred records: wave-cooperative global-memory path -----------------------------
  if (!(dbg(p) & 4)) {
    const u32 nd = sm.ndefer < MAX_DEFER ? sm.ndefer : MAX_DEFER;
    WaveAcc wa;
    wa.g = p.data; wa.end = p.end; wa.eof = p.eof; wa.lane = lane; wa.front = p.front;
    for (u32 i = wid; i < nd; i += NWAVES) {
      const u64 s = sm.defer_s[i], k = sm.defer_k[i], aux = sm.defer_aux[i];
      u64 len = 0, epos = 0, elen = 0;
      // inline: an out-of-line call here saved ~5 KB of registers to scratch per tile
      const u32 st = run_record<F>(wa, s, aux, len, epos, elen);
      if (lane == 0) {
        if (st == ST_OK) put_row(p, k, s, len);
        else note_bad(bad, k, tile, st, p.base + epos, elen);
      }
    }
  }

  // ---- first bad record of the tile -> slab-wide min ----------------------------------------
  if (ts) ts[6] = stamp();
  if (bad.key != KEY_NONE) atomicMin(&sm.badkey, bad.key);
  lds_barrier();
  const u64 tkey = sm.badkey;
  if (tkey != KEY_NONE) {
    if (bad.key == tkey) {
      p.detail[2 * (u64)tile] = bad.pos;
      p.detail[2 * (u64)tile + 1] = bad.len;
    }
    if (tid == 0) atomicMin(p.badkey, tkey);  // one device-scope atomic per tile with a bad record
  }
}

// stage a loaded tile: raw bytes + per-byte class masks into LDS
template <int F, class SM>
__device__ __forceinline__ void stage_tile(SM &sm, const uint4 (&v)[CPT + 1], int tid) {
  uint16_t *mnl16 = reinterpret_cast<uint16_t *>(sm.mnl);
  uint16_t *mx16 = reinterpret_cast<uint16_t *>(sm.mx);
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const u32 c = (u32)(k * NTHREADS + tid);
    *reinterpret_cast<uint4 *>(&sm.raw[FRONT + c * CHUNK]) = v[k];
    mnl16[c] = (uint16_t)eq16(v[k], '\n');
    if (Traits<F>::kX) mx16[c] = (uint16_t)eq16(v[k], Traits<F>::xc);
  }
  if (tid < HALO_CHUNKS) {
    const u32 c = (u32)(CPT * NTHREADS + tid);
    *reinterpret_cast<uint4 *>(&sm.raw[FRONT + c * CHUNK]) = v[CPT];
    mnl16[c] = (uint16_t)eq16(v[CPT], '\n');
    if (Traits<F>::kX) mx16[c] = (uint16_t)eq16(v[CPT], Traits<F>::xc);
  } else if (tid == HALO_CHUNKS) {
    *reinterpret_cast<uint4 *>(&sm.raw[0]) = v[CPT];
  }
}

// k_tile_agg<F>: pass 1 of a two-pass build -- the monoid aggregate of every tile (bytes
// [tlo, thi) only), no staging of the raw bytes: 16-B/lane loads -> per-chunk class masks in
// LDS -> per-thread 128-byte regions in byte order -> ordered block reduce.
template <int F>
__global__ __launch_bounds__(NTHREADS) void k_tile_agg(const SlabParams p, u64 *agg) {
  typedef typename Traits<F>::M M;
  __shared__ u64 mnl[TILE / 64], mx[Traits<F>::kX ? TILE / 64 : 1], wtot[NWAVES];
  // a wrongly speculated format: the two-pass kernels exit like the tile passes
  if (gated_off(p)) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const u64 tile = blockIdx.x, tlo = tile * TILE;
  const u32 tlen = (u32)(((tlo + TILE < p.n) ? tlo + TILE : p.n) - tlo);
  const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(p.data + tlo), (short)0, (int)tlen, 0x00020000);
  uint4 v[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k)
    v[k] = to_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, (int)((u32)(k * NTHREADS + tid) * CHUNK), 0, 0));
  if (tlen & 3u) {  // the slab's last dword is partial: its bytes one by one
    const u32 w = tail_dword(rs, tlen);
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const u32 off = (u32)(k * NTHREADS + tid) * CHUNK;
      if (off < tlen && off + CHUNK > tlen) patch_tail(v[k], off, tlen, w);
    }
  }
  uint16_t *m16 = reinterpret_cast<uint16_t *>(mnl), *x16 = reinterpret_cast<uint16_t *>(mx);
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const u32 c = (u32)(k * NTHREADS + tid);
    m16[c] = (uint16_t)eq16(v[k], '\n');
    if (Traits<F>::kX) x16[c] = (uint16_t)eq16(v[k], Traits<F>::xc);
  }
  __syncthreads();
  const u32 rlo = (u32)tid * REGION;
  const u32 len0 = tlen > rlo ? (tlen - rlo >= 64 ? 64u : tlen - rlo) : 0u;
  const u32 len1 = tlen > rlo + 64 ? (tlen - rlo - 64 >= 64 ? 64u : tlen - rlo - 64) : 0u;
  const u64 nl0 = mnl[2 * tid] & lowmask(len0), nl1 = mnl[2 * tid + 1] & lowmask(len1);
  const u64 x0 = Traits<F>::kX ? mx[2 * tid] & lowmask(len0) : 0, x1 = Traits<F>::kX ? mx[2 * tid + 1] & lowmask(len1) : 0;
  const u64 ragg = M::combine(M::seg(nl0, x0, len0), M::seg(nl1, x1, len1));
  const u64 incl = wave_incl_scan<M>(ragg, lane);
  if (lane == 63) wtot[wid] = incl;
  __syncthreads();
  if (tid == 0) {
    u64 t = M::identity();
    for (int w = 0; w < NWAVES; ++w) t = M::combine(t, wtot[w]);
    agg[tile] = t;
  }
}

// the slab aggregate of a two-pass build, where k_finalize reads it (last status word)
__global__ void k_tile_total(const SlabParams p, const u64 *agg, const u64 *excl, int fmt) {
  if (threadIdx.x || blockIdx.x || gated_off(p)) return;
  const u64 t = p.ntiles - 1;
  u64 tot;
  if (fmt == F_FASTA) tot = FastaMonoid::combine(excl[t], agg[t]);
  else if (fmt == F_SAM) tot = SamMonoid::combine(excl[t], agg[t]);
  else tot = CountMonoid::combine(excl[t], agg[t]);
  ((u64 *)p.status)[t] = FLAG_INC | ((u64)p.epoch << EPOCH_SHIFT) | tot;
}

// k_index1<F>: one tile per workgroup (grid = ntiles), no register prefetch: latency is
// hidden by the other workgroups resident on the CU rather than inside the workgroup.
template <int F>
__global__ __launch_bounds__(NTHREADS) void k_index1(const SlabParams p) {
  __shared__ Smem<F> sm;
  if (gated_off(p)) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const u32 tile = blockIdx.x;
  const bool timing = tmg(p) && tid == 0;
  u64 tsb[8];
  if (timing) tsb[0] = stamp();
  {
    uint4 v[CPT + 1];
    load_tile_buf(p, tile, tid, v);
    trim_tile(p, tile, tid, v);
    stage_tile<F>(sm, v, tid);
  }
  lds_barrier();
  if (timing) tsb[7] = stamp();
  process_tile<F>(p, (gu64 *)p.status, tile, sm, tid, lane, wid, timing ? tsb : nullptr);
  if (timing) {  // diagnostic: phase sums into 65536 slots (summed by the host)
    const u64 te = stamp();
    u64 *o = tmg(p) + (u64)(blockIdx.x & 65535) * 9;
    atomicAdd(&o[0], tsb[7] - tsb[0]);
    atomicAdd(&o[1], tsb[1] - tsb[7]);
    atomicAdd(&o[2], tsb[2] - tsb[1]);
    atomicAdd(&o[3], tsb[3] - tsb[2]);
    atomicAdd(&o[4], tsb[4] - tsb[3]);
    atomicAdd(&o[5], tsb[5] - tsb[4]);
    atomicAdd(&o[6], te - tsb[5]);
    atomicAdd(&o[8], 1ull);
  }
}


// ====================================================================================
// Tile-pass building blocks (k_fq_tiles / k_fa_tiles / k_line_tiles): result encodings,
// the k_fixup queue, the LDS certifiers and the device-scope atomics they use.
// ====================================================================================
// ASCII bytes.TrimSpace bounds of r[lo, hi); false if a byte >= 0x80 decides (Unicode path)
__device__ __forceinline__ bool trim_ascii(const uint8_t *r, u32 lo, u32 hi, u32 &tl, u32 &th) {
  while (lo < hi) {
    const u32 c = r[lo];
    if (c >= 0x80) return false;
    if (!ascii_space(c)) break;
    ++lo;
  }
  while (hi > lo) {
    const u32 c = r[hi - 1];
    if (c >= 0x80) return false;
    if (!ascii_space(c)) break;
    --hi;
  }
  tl = lo; th = hi;
  return true;
}

// FastaMonoid::combine on 32-bit aggregates (a wave's count of '>' fits 13 bits)
__device__ __forceinline__ u32 fa_comb32(u32 a, u32 b) {
  const u32 af = a & 3u, bf = b & 3u;
  const u32 bd = (b >> 2) & 1u;
  const u32 cnt = (a >> 3) + (b >> 3) + ((af == 2u) ? bd : 0u);
  const u32 d = af == 0u ? bd : (a >> 2) & 1u;
  const u32 f = bf == 0u ? af : bf;
  return (cnt << 3) | (d << 2) | f;
}
__device__ __forceinline__ u32 wave_scan_fa32(u32 v) { SIDX_DPP_SCAN(v, fa_comb32); return v; }

// bytes that differ between raw[a, a+4) and raw[b, b+4) (only the first n if n < 4);
// aligned dword LDS reads + v_alignbyte (raw is 4-aligned)
__device__ __forceinline__ u32 lds_diff4(const uint8_t *raw, u32 a, u32 b, u32 n) {
  const u32 *w = reinterpret_cast<const u32 *>(raw);
  const u32 wa = __builtin_amdgcn_alignbyte(w[(a >> 2) + 1], w[a >> 2], a & 3);
  const u32 wb = __builtin_amdgcn_alignbyte(w[(b >> 2) + 1], w[b >> 2], b & 3);
  const u32 m = n >= 4 ? ~0u : ((1u << (8 * n)) - 1u);
  return (wa ^ wb) & m;
}


// fastq.go:134-213 certifies the record [s, e3] valid (the common case) when its TrimSpace
// edges are printable ASCII, LF or CRLF line ends: branch-free over the 13 edge bytes (one
// LDS round).  Anything else -- an error, a blank or space-padded line, a byte >= 0x80 at an
// edge -- returns false and the record goes to k_fixup, whose general validator reports
// exactly what Go reports.  A plus line that carries an ID comes back with cn = the ID length:
// r[s+1, s+1+cn) must then equal r[cb, cb+cn) (the caller compares).  r: the tile's byte 0.
#pragma clang diagnostic ignored "-Wbitwise-instead-of-logical"  // the flags below are combined branch-free
__device__ __forceinline__ bool fq_ok(const uint8_t *r, u32 s, u32 e0, u32 e1, u32 e2, u32 e3, u32 &cn, u32 &cb,
                                      u32 &crs, bool &idclean) {
  const u32 cs = r[s], ci1 = r[s + 1], cs1 = r[e0 + 1], cp = r[e1 + 1], cq1 = r[e2 + 1];
  const u32 a0 = r[e0 - 1], a1 = r[e1 - 1], a2 = r[e2 - 1], a3 = r[e3 - 1];
  const u32 b0 = r[e0 - 2], b1 = r[e1 - 2], b2 = r[e2 - 2], b3 = r[e3 - 2];
  // a '\r' before the '\n' is trimmed too: z = the end of the line's trimmed content
  const u32 c0 = a0 == '\r', c1 = a1 == '\r', c2 = a2 == '\r', c3 = a3 == '\r';
  const u32 z0 = e0 - c0, z1 = e1 - c1, z2 = e2 - c2, z3 = e3 - c3;
  const u32 l0 = c0 ? b0 : a0, l1 = c1 ? b1 : a1, l2 = c2 ? b2 : a2, l3 = c3 ? b3 : a3;
  const bool pluslong = z2 > e1 + 2;  // TrimSpace(plus) longer than "+": the ID must match
  const bool ok = (e0 > s + 1) & (cs == '@') & (cp == '+') &                   // :164-169, :191
                  (z1 > e0 + 1) & ascii_nonspace(cs1) & ascii_nonspace(l1) &   // seq content
                  (z3 > e2 + 1) & ascii_nonspace(cq1) & ascii_nonspace(l3) &   // qual content
                  (z1 - e0 == z3 - e2) &                                       // :202-207
                  ascii_nonspace(l2) &                                         // plus edge
                  (!pluslong | (ascii_nonspace(ci1) & ascii_nonspace(l0) & (z0 - s == z2 - e1 - 1)));
  cn = (ok && pluslong) ? z0 - s - 1 : 0u;  // :195-199 ID bytes r[s+1..] vs r[e1+2..]
  cb = e1 + 2;
  crs = c0 | (c1 << 1) | (c3 << 2);  // (filters) the '\r' before the ID / sequence / quality line ends
  idclean = ascii_nonspace(ci1) & ascii_nonspace(l0) & (z0 > s + 1);  // TrimSpace(ID) drops only the line end
  return ok;
}

// FASTQ phase read off the tile: the first newline c (of the first 16) after which an
// '@' line, a sequence line, a '+' line and an equal-length quality line follow.
// (plane: the lane number for the predicate, TilePred)
__device__ __forceinline__ u32 fq_guess_at(const uint8_t *raw, const uint16_t *nlpos, u32 TT, int lane, int plane) {
  // branch-free: every lane reads (clamped indices, values ignored where not valid), so the
  // two LDS rounds are not serialised behind branches
  const u32 c = (u32)lane & 15u;
  const u32 a = nlpos[c], b1 = nlpos[c + 1], b2 = nlpos[c + 2], b3 = nlpos[c + 3], b4 = nlpos[c + 4];
  const u32 x = raw[FRONT + a + 1], y = raw[FRONT + b2 + 1];
  const bool ok = ((u32)plane < 16) & (c + 4 < TT) & (x == '@') & (y == '+') & (b2 - b1 > 1) & ((b2 - b1) == (b4 - b3));
  const u64 m = __ballot(ok);
  return m ? (ctz64(m) & 3u) : GUESS_NONE;
}

// Device-scope atomics and stores through address-space-1 pointers: a generic (flat) access
// inside the streaming loop would make the compiler drain every outstanding load, the tile
// DMA included, before the next LDS access (a flat access may touch LDS).
typedef __attribute__((address_space(1))) u32 gu32;
__device__ __forceinline__ u32 g_add(u32 *p, u32 v) {
  return __hip_atomic_fetch_add((gu32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void g_or(u32 *p, u32 v) {
  (void)__hip_atomic_fetch_or((gu32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void g_min64(u64 *p, u64 v) {
  (void)__hip_atomic_fetch_min((__attribute__((address_space(1))) u64 *)p, v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

// The claim loop of a persistent tile pass (k_fq_tiles, k_fa_tiles; the plan: sidx_claim.hpp).
// A workgroup's first claim is its block index; every later one is G + a ticket of counters[6]
// (zero at a build's start like the other counters: the previous build's finalize, or the host's
// reset of a dirty slot).  Tickets rise, so claims start in file order, and claims G.. go to
// whichever workgroup asks first.  body(t, r) runs one tile of the claim r = [tb, te) and holds
// at least one workgroup barrier.
//
// The ticket's latency (1-3 us under the streaming load, against ~5 us per tile) is hidden:
// thread 0 issues the atomic CLAIM_AHEAD tiles before the claim's end (at its first tile when it
// is shorter), right before that tile's DMA, so the wait the tile makes for its DMA anyway --
// the explicit s_waitcnt vmcnt(0) in the body -- covers the ticket too.  The DMA is inline asm the
// compiler does not count, so to the compiler the ticket is the only load in flight and it puts a
// vmcnt(0) of its own before the first read of `nx`: that read is therefore placed before the
// *next* tile's DMA issue, after the explicit wait of the tile the ticket travelled with, where
// nothing is left to wait for.  There thread 0 writes the ticket to one word of the workgroup's
// LDS block (`word`); the barriers of that tile and the later ones publish it, and every wave
// reads it after the claim's last tile.  The word is written again only after a barrier of the
// next claim, which no wave reaches before it has read the word.  No barrier is added.
// Every claim but the plan's last has two tiles or more (claim_plan), which this needs; after
// the last claim every ticket is past the end, so its workgroup asks for none.
//
// Registers.  The tile loop keeps no SlabParams field live: left to itself the compiler hoists every
// field, every 64-bit bound and every thread predicate the body touches out of the loop, runs out of
// scalar registers and reloads them from spill lanes between every pair of barriers.  So
//   * the kernel's parameters are read where they are used through kargs(), the kernel argument
//     block behind a pointer the compiler cannot see through (scalar loads that hit the constant
//     cache): once per claim for the plan and the claim's bytes, and in the cold branches of a tile;
//   * a tile's bounds are 32-bit offsets from its claim's first byte (ClaimBytes: a claim holds at
//     most CLAIM_BMAX tiles);
//   * the thread predicates of a tile (tid == 0, lane == 63, wid == 3 ...) are taken from copies of
//     tid / lane / wid made opaque once per tile (TilePred): one compare where each is used.
constexpr u32 CLAIM_AHEAD = 8;  // tiles before a claim's end at which its workgroup asks for the next
typedef const __attribute__((address_space(4))) SlabParams *KArgs;
// the kernel's SlabParams (its only parameter, at offset 0 of the argument block)
__device__ __forceinline__ KArgs kargs() {
  KArgs k = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}
struct TilePred {
  int tid, lane, wid;
};
__device__ __forceinline__ TilePred tile_pred(int tid, int lane, int wid) {
  TilePred q = {tid, lane, wid};
  asm volatile("" : "+v"(q.tid), "+v"(q.lane), "+s"(q.wid));
  return q;
}
constexpr u32 CLAIM_SAT = (CLAIM_BMAX + 2) * (u32)TILE;  // past any offset a claim's tiles reach
struct ClaimBytes {
  const uint8_t *base;  // the claim's first byte: data + tb * TILE
  u32 nrel, erel;       // the slab's owned (n) and readable (end) bytes from base on, at most CLAIM_SAT
  // tile `rel` of the claim: the bytes it owns and the bytes readable from its first byte on
  __device__ __forceinline__ u32 tlen(u32 rel) const { return umin(nrel - rel * TILE, (u32)TILE); }
  __device__ __forceinline__ u32 llen(u32 rel) const { return umin(erel - rel * TILE, (u32)(TILE + SHALO)); }
};
// tile t has fewer than FRONT readable bytes in front of it (the slab's first tile only)
__device__ __forceinline__ bool tile_nofront(u32 t) { return t == 0 && kargs()->front < FRONT; }
template <class Body>
__device__ __forceinline__ void claim_loop(u32 &word, int tid, Body &&body) {
  u32 nx = 0;  // thread 0: the next claim's ticket
  for (u32 c = blockIdx.x;;) {
    const KArgs k = kargs();
    const ClaimPlan cp = claim_plan(k->ntiles, k->pgrid);
    if (c >= cp.nclaims) break;
    const ClaimRange r = claim_range(cp, c);
    const u32 more = (u32)__builtin_amdgcn_readfirstlane((int)(c + 1 < cp.nclaims));  // (one scalar, no lane mask)
    const u32 ta = r.te - r.tb > CLAIM_AHEAD ? r.te - CLAIM_AHEAD : r.tb;
    const u64 lo = (u64)r.tb * TILE, nleft = k->n - lo, eleft = k->end - lo;
    ClaimBytes cb;
    cb.base = k->data + lo;
    cb.nrel = nleft < CLAIM_SAT ? (u32)nleft : CLAIM_SAT;
    cb.erel = eleft < CLAIM_SAT ? (u32)eleft : CLAIM_SAT;
    for (u32 t = r.tb; t < r.te; ++t) {
      if (more && t - ta <= 1u) {  // t == ta or ta + 1 (uniform: the predicate below is not kept over the loop)
        int t0 = tid;
        asm volatile("" : "+v"(t0));
        if (t0 == 0) {
          if (t == ta) {
            // (an offset the compiler cannot see through: on an address it knows to be uniform it
            // would fold the lanes' adds into one and read the result back with a readfirstlane --
            // and a wait for the ticket -- right here, ahead of the DMA)
            u32 z = 0;
            asm("" : "+v"(z));
            nx = g_add(&kargs()->counters[6] + z, 1u);
          } else {
            word = nx;
          }
        }
      }
      body(t, r, cb);
    }
    if (!more) break;
    c = kargs()->pgrid + (u32)__builtin_amdgcn_readfirstlane((int)word);
  }
}

__device__ __forceinline__ void push_fix(const SlabParams &p, u64 start, u64 g, u32 tile) {
  const u32 i = g_add(&p.counters[2], 1u);
  if (i < p.fixcap) {
    gu64 *f = (gu64 *)(p.fix + (sizeof(FixRec) / sizeof(u64)) * (u64)i);
    f[0] = start; f[1] = g; f[2] = tile;  // FixRec {start, g, tile, pad}
  } else {
    g_or(&p.counters[3], 1u);  // overflow: the host re-runs the build on the general kernel
  }
  if (start == ~0ull) (void)g_add(&p.counters[3], 2u);  // whole-tile items (diagnostic), bits 1..
}


// ====================================================================================
// FASTQ tile pass: k_fq_tiles -> exclusive scan of the tile newline counts -> k_fq_place.
// LDS-DMA staging, '\n' masks, newline positions, the phase read off the tile, lane
// validation with fq_ok -- and no cross-workgroup dependency at all: each tile's valid records go to a provisional row table (start |
// length << 16, indexed by the tile-local record number) and its newline count to agg[t].
// Once every count is known, a device-wide scan gives each tile's true newline rank j0, and
// k_fq_place writes the final rows at their global record numbers (or queues the tile for
// k_fixup when the phase guess was wrong).  Extra traffic: 4 bytes per record
// written and read back (about 2 % of the input for short-read FASTQ).
// ====================================================================================
// Per-tile results.  Every byte this pass writes is expensive next to the bytes it streams in
// (tools/streambench.hip: 32 bytes per 16 KiB tile cost 4 % of the pass, 228 bytes 10 %), so a
// tile writes one u64 (tile_agg[t]: fq_word, sidx_device.hpp; the scan reads its newline count) and one u16
// per record (its start, bit 15 = not certified) plus the end of the last record -- a record's
// length is the next one's start minus its own (the records of a tile are back to back).
// Deferred records (dl[], ds[]: 2 * MAX_DEFER words per tile) are written only when a tile
// defers.
// (the word: fq_word / fq_unpack, sidx_device.hpp)
// Where a tile's u16 starts are (round 6): tile t's first FQ_LINE_E entries in one 128-byte line
// at entry FQ_LINE_E t of tile_stage -- a dense, tile-indexed array that advances with the read
// stream, one full-line store per tile -- and entries FQ_LINE_E.. (tiles of more than 63
// records; C2 has ~47 per tile) in an overflow slot of FQ_OVF entries per tile behind the lines.
// History: a fixed 1 KiB slot per tile (round 3-4) left a partial line per tile;
// round 5 appended each workgroup's arrays to a region of its own through an LDS ring flushed in
// whole lines, packed at any entry (the offset in the tile word).  Both run the same as this
// layout on an input buffer the box places well and ~0.2 ms slower on one it places badly
// (profiles/r06/calls/a: 1.866-1.871 against 1.874-1.882 ms on three fast copies, 2.086 against
// 2.102 on the slow one; whole builds 2.005-2.013 against 2.000-2.008, 2.227 against 2.228) --
// this one needs no ring, no regions and no offset field.  Round 5 also dropped: a tile's stores
// issued after the next tile's DMA, two LDS slots per workgroup (4 workgroups per CU), fewer
// records certified per wave, temporal row-start stores (all slower or within noise).
constexpr u32 FQ_LINE_E = 64;                                // u16 entries per line
constexpr u32 FQ_OVF = ((RCAP + 1 - FQ_LINE_E) + 7u) & ~7u;  // overflow entries per tile (16-byte multiple)
__device__ __forceinline__ u64 fq_ovf(const SlabParams &p, u64 t) { return (u64)p.ntiles * FQ_LINE_E + t * FQ_OVF; }
// entry L of tile t (L <= nrec: entry nrec is the end of the tile's last record)
__device__ __forceinline__ u32 fq_start(const SlabParams &p, u64 t, u32 L) {
  const uint16_t *s = reinterpret_cast<const uint16_t *>(p.tile_stage);
  return L < FQ_LINE_E ? s[t * FQ_LINE_E + L] : s[fq_ovf(p, t) + (L - FQ_LINE_E)];
}
constexpr u32 FQ_UNCERT = 0x8000;  // row entry: the record is not certified here
__device__ __forceinline__ u32 *fq_defer(const SlabParams &p, u64 t) { return p.tile_words + t * (2 * MAX_DEFER); }

// A workgroup keeps the lines and tile words of FQ_BLK consecutive tiles in LDS, so they leave as
// one 2 KiB burst of lines and one 128-byte line of words per FQ_BLK tiles (profiles/r06/calls/e:
// the kernel 1.872 -> 1.855 ms and the build 1.998 -> 1.982 on each of four input copies, against
// one tile per burst).  The tiles come in claims of up to CLAIM_BMAX consecutive tiles that the
// workgroups take in file order (k_fq_tiles, sidx_claim.hpp); a claim's bursts start at its first
// tile, and one shorter than FQ_BLK tiles leaves at the claim's end.
#ifndef SIDX_FQ_BLK
#define SIDX_FQ_BLK 16
#endif
constexpr u32 FQ_BLK = SIDX_FQ_BLK;
static_assert(CLAIM_BMIN % 2 == 0 && FQ_BLK % 2 == 0,
              "claims, and so bursts, start at even tiles: the tile words leave 16 bytes per lane");
static_assert(CLAIM_BMAX <= 32, "a claim holds at most 32 tiles (the batch size measured best)");
struct __align__(16) TilesSmem {
  uint16_t nlpos[SNLCAP + 8];        // + 8: the certifier reads aligned 8-entry windows
  uint16_t line[FQ_BLK][FQ_LINE_E];  // the batch's lines: a tile's first FQ_LINE_E entries each
  u64 words[FQ_BLK];                 // the batch's tile words
  u32 wtot[SNW];
  u32 nh, ndefer, slow, pad;
};

// entry L of the tile being certified (batch slot j): its line in LDS, or the overflow slot (a tile
// of more than 63 records: the slot's address is read off the kernel arguments there)
__device__ __forceinline__ void fq_put(TilesSmem &S, u32 t, u32 j, u32 L, uint16_t v) {
  if (L < FQ_LINE_E) {
    S.line[j][L] = v;
  } else {
    const KArgs k = kargs();
    uint16_t *ovf = reinterpret_cast<uint16_t *>(k->tile_stage) + ((u64)k->ntiles * FQ_LINE_E + (u64)t * FQ_OVF);
    __builtin_nontemporal_store(v, ovf + (L - FQ_LINE_E));
  }
}
// the buffer descriptor of tile_rsrc from a tile's first byte and its readable length
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc_at(const uint8_t *tile0, u32 llen) {
  const u64 ba = (u64)tile0;
  const uint8_t *sbase = (const uint8_t *)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)ba)) |
                                           ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(ba >> 32)) << 32));
  return __builtin_amdgcn_make_buffer_rsrc((void *)sbase, (short)0, (int)__builtin_amdgcn_readfirstlane((int)llen),
                                           0x00020000);
}

template <bool kSpans>
__device__ __forceinline__ void tiles_iter(const SlabParams &p, const ClaimBytes &cb, u32 rel, TilesSmem &S,
                                           uint8_t *raw, u32 t, int tid, int lane, int wid, u64 *tacc, u32 j,
                                           bool flush) {
  // diagnostic phase stamps (SIDX_DIAG builds with SHOCKIDX_TIMING; tacc == nullptr otherwise):
  // lane 0 of waves 0 (the certifying wave) and 1 accumulate the cycles of each phase
  u64 tprev = tacc ? stamp() : 0;
  const TilePred q_ = tile_pred(tid, lane, wid);  // (predicates only: addresses use tid / lane / wid)
  const int ptid = q_.tid, plane = q_.lane, pwid = q_.wid;
  const u32 tlen = cb.tlen(rel), llen = cb.llen(rel);
  const uint8_t *tile0 = cb.base + rel * (u32)TILE;
  const bool nofront = tile_nofront(t);
#define TILES_STAMP(i)              \
  if (tacc) {                       \
    const u64 tn_ = stamp();        \
    tacc[i] += tn_ - tprev;         \
    tprev = tn_;                    \
  }
  // ---- P0 / P1: DMA of this tile; each wave waits for its own pieces ------------------------
  // wave priorities: a tile's DMA is issued ahead of other workgroups' compute, and a tile's
  // record certification (one wave, the tile's critical path while its other waves wait at the
  // barrier) ahead of other workgroups' mask / position phases -- each workgroup then returns
  // its slot to the DMA sooner (10 GiB: 2.24-2.31 -> 2.09 ms)
  __builtin_amdgcn_s_setprio(3);
  stage_tile_at<true>(tile0, llen, !nofront, (u32)(size_t)(lds_u8 *)raw, wid, lane, plane);
  __builtin_amdgcn_s_setprio(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TILES_STAMP(0);
  // the last wave also collects the newlines past the tile: the straggler at the next barrier,
  // so it goes first
  if (pwid == SNW - 1) __builtin_amdgcn_s_setprio(1);
  if (llen < (u32)(TILE + SHALO) || nofront) {  // slab end / file start: zero-fill
    lds_barrier();  // (every wave's DMA landed: the fill may touch any part of the slot)
    for (u32 c = (u32)tid; c < (u32)((TILE + SHALO) / 16); c += SNT) {
      const u32 o = c * 16;
      if (o + 16 <= llen) continue;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (o < llen) {
        v = keep_bytes(*reinterpret_cast<const uint4 *>(raw + FRONT + o), llen - o);
        if (llen & 3u) {
          const auto rs = tile_rsrc_at(tile0, llen);
          patch_tail(v, o, llen, tail_dword(rs, llen));
        }
      }
      *reinterpret_cast<uint4 *>(raw + FRONT + o) = v;
    }
    if (nofront && ptid == 0) *reinterpret_cast<uint4 *>(raw) = make_uint4(0, 0, 0, 0);
    lds_barrier();
  }
  // ---- P2: '\n' mask word per thread (swizzled 16-byte reads), block count ----------------
  u64 m = 0;  // 3-op equality flags; the rare suspect word ("\n\v") is re-checked exactly
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u32 cj = ((u32)j + ((u32)tid >> 2)) & 3u;
    const uint4 v = *reinterpret_cast<const uint4 *>(raw + FRONT + tid * 64 + 16 * cj);
    m |= (u64)eq16x(v, '\n') << (16 * cj);
  }
  if (eq_suspect(m)) {
    m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) m |= (u64)eq16(*reinterpret_cast<const uint4 *>(raw + FRONT + tid * 64 + 16 * j), '\n') << (16 * j);
  }
  const u32 rl = tlen > (u32)tid * 64 ? tlen - (u32)tid * 64 : 0u;
  const u64 mown = m & lowmask(rl);
  const u32 c = popc64(mown);
  // (fewer VALU instructions per tile -- the pass issues VALU about two thirds of its time: a
  // ballot scan of the small per-lane counts, the wave totals read as scalars, a word's first two
  // positions without the loop, the halo words by the 3-op equality flags; round 5, within noise)
  const u32 incl = wave_scan_add_small(c);
  if (plane == 63) S.wtot[(u32)tid >> 6] = incl;  // (the address in a vector register: scalar ones are short)
  if (ptid == 0) { S.ndefer = 0; S.slow = 0; }
  lds_barrier();
  TILES_STAMP(1);
  static_assert(SNW == 4, "the wave totals: one uniform 16-byte LDS read");
  const uint4 w4 = *reinterpret_cast<const uint4 *>(S.wtot);
  const u32 t0 = (u32)__builtin_amdgcn_readfirstlane((int)w4.x), t1 = (u32)__builtin_amdgcn_readfirstlane((int)w4.y),
            t2 = (u32)__builtin_amdgcn_readfirstlane((int)w4.z), t3 = (u32)__builtin_amdgcn_readfirstlane((int)w4.w);
  const u32 T = t0 + t1 + t2 + t3;
  const u32 wpre = (pwid > 0 ? t0 : 0u) + (pwid > 1 ? t1 : 0u) + (pwid > 2 ? t2 : 0u);
  // ---- P3: newline positions (tile + the first NLHALO past it), phase, validation -----------
  const bool use_arr = T + NLHALO <= (u32)SNLCAP;
  if (use_arr) {
    u32 o = wpre + incl - c;
    u64 mm = mown;
    const u64 m1 = mm & (mm - 1);  // a word's first two '\n' without the loop
    if (c >= 1) S.nlpos[o] = (uint16_t)((u32)tid * 64 + ctz64(mm));
    if (c >= 2) S.nlpos[o + 1] = (uint16_t)((u32)tid * 64 + ctz64(m1));
    mm = m1 & (m1 - 1);
    o += 2;
    while (mm) {
      S.nlpos[o++] = (uint16_t)((u32)tid * 64 + ctz64(mm));
      mm &= mm - 1;
    }
    if (pwid == SNW - 1) {
      const u32 wb = tlen >> 6;
      u32 hc = 0;
      u64 hm = 0;
      const u32 wd = wb + (u32)lane;
      if (wd * 64 < llen) {
        // this lane's word past the tile's last byte, classified here from the slot (the halo
        // DMA was other waves'; no mask words are kept in LDS)
#pragma unroll
        for (int j = 0; j < 4; ++j) hm |= (u64)eq16x(*reinterpret_cast<const uint4 *>(raw + FRONT + wd * 64 + 16 * j), '\n') << (16 * j);
        if (eq_suspect(hm)) {
          hm = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            hm |= (u64)eq16(*reinterpret_cast<const uint4 *>(raw + FRONT + wd * 64 + 16 * j), '\n') << (16 * j);
        }
        if (plane == 0) hm &= ~lowmask(tlen & 63);  // (wd == wb)
        if (wd * 64 + 64 > llen) hm &= lowmask(llen - wd * 64);
        hc = popc64(hm);
      }
      const u32 hpre = wave_scan_add_small(hc);
      u32 o2 = hpre - hc;
      while (hm && o2 < (u32)NLHALO) {
        S.nlpos[T + o2] = (uint16_t)(wd * 64 + ctz64(hm));
        ++o2;
        hm &= hm - 1;
      }
      if (plane == 63) S.nh = hpre < (u32)NLHALO ? hpre : (u32)NLHALO;
    }
  }
  lds_barrier();
  TILES_STAMP(2);
  bool fs = false;  // the file's first tile
  const u32 TT = use_arr ? T + S.nh : 0;
  u32 gi0;
  if (t == 0) {  // slab start: rank known
    const KArgs k = kargs();
    fs = k->file_start != 0;
    gi0 = (u32)((3 - (k->state_in & 3)) & 3);
  } else if (use_arr && (pwid == 0 || (T + 3) / 4 + 1 > 64u * (u32)pwid)) {
    gi0 = fq_guess_at(raw, S.nlpos, TT, lane, plane);
  } else {
    gi0 = GUESS_NONE;  // (or this wave has no records to certify: only wave 0's gi0 is kept)
  }
  const u32 ng = gi0 < T ? (T - gi0 + 3) / 4 : 0;
  const u32 nrec = ng + (fs ? 1u : 0u);
  const bool slow = !use_arr || gi0 == GUESS_NONE || nrec > (u32)RCAP;
  __builtin_amdgcn_s_setprio(2);
  if (!slow) {
    // record q = 64 w + lane (a tile's ~50 records fit one wave); one LDS round per step
    const uint8_t *r = raw + FRONT;
    for (u32 qb = (u32)wid * 64u; qb < ng + 1; qb += SNW * 64u) {
      const u32 q = qb + (u32)lane;
      const bool inr = q < ng;
      const bool act = inr || (q == ng && fs);
      const u32 d = inr ? gi0 + 4 * q : 0u;
      const u32 i = inr ? d + 1 : 0u;
      const u32 L = inr ? q + (fs ? 1u : 0u) : 0u;
      const bool known = act && i + 3 < TT;
      u32 s0, e0, e1, e2, e3;
      if (!fs) {
        // nlpos[d .. d+4] from two aligned 8-byte reads: d & 3 = gi0 & 3 is the same in every lane
        const u32 db = inr ? (d & ~3u) : 0u;  // s0 is needed even when the record runs past the halo (k_fixup)
        const uint2 wa = *reinterpret_cast<const uint2 *>(&S.nlpos[db]);
        const uint2 wb = *reinterpret_cast<const uint2 *>(&S.nlpos[db + 4]);
        const u32 sh2 = (gi0 & 1u) * 2u;   // byte shift inside a dword
        const bool hiw = (gi0 & 2u) != 0u;  // start in the second dword
        const u32 x0 = hiw ? wa.y : wa.x, x1 = hiw ? wb.x : wa.y, x2 = hiw ? wb.y : wb.x, x3 = hiw ? 0u : wb.y;
        const u32 p01 = __builtin_amdgcn_alignbyte(x1, x0, sh2), p23 = __builtin_amdgcn_alignbyte(x2, x1, sh2),
                  p4 = __builtin_amdgcn_alignbyte(x3, x2, sh2);
        s0 = inr ? (p01 & 0xFFFFu) + 1u : 0u;
        e0 = known ? p01 >> 16 : 0u;
        e1 = known ? p23 & 0xFFFFu : 0u;
        e2 = known ? p23 >> 16 : 0u;
        e3 = known ? p4 & 0xFFFFu : 0u;
      } else {  // the file's first tile: record 0 starts at offset 0, its line ends are entries 0..3
        const u32 ic = known ? i : 0u;
        e0 = S.nlpos[ic]; e1 = S.nlpos[ic + 1]; e2 = S.nlpos[ic + 2]; e3 = S.nlpos[ic + 3];
        s0 = inr ? S.nlpos[d] + 1u : 0u;
      }
      u32 cn = 0, cb = 0, crs = 0;
      bool idclean = false;
      const bool ok = fq_ok(r, s0, e0, e1, e2, e3, cn, cb, crs, idclean) && known;
      bool good = ok;
      const u32 ca = FRONT + s0 + 1;
      cb += FRONT;
      const bool need = ok && cn != 0;
      bool idmis = false;
      {  // plus-line IDs: per lane up to 64 bytes, longer ones by the whole wave
        if (__ballot(need && cn <= 64)) {
          u32 diff = 0;
          const u32 nn = (need && cn <= 64) ? cn : 0u;
          for (u32 o = 0; o < nn; o += 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const u32 oo = o + 4 * (u32)j;
              if (oo < nn) diff |= lds_diff4(raw, ca + oo, cb + oo, nn - oo);
            }
          }
          idmis = diff != 0;
        }
        u64 mc = __ballot(need && cn > 64);
        while (mc) {
          const int Lc = (int)ctz64(mc);
          mc &= mc - 1;
          const u32 xa = (u32)__shfl((int)ca, Lc, 64), xb = (u32)__shfl((int)cb, Lc, 64);
          const u32 xn = (u32)__shfl((int)cn, Lc, 64);
          u32 diff = 0;
          for (u32 o = (u32)lane * 4; o < xn; o += 256) diff |= lds_diff4(raw, xa + o, xb + o, xn - o);
          const bool any = __ballot(diff != 0) != 0;
          if (lane == Lc) idmis = any;
        }
      }
      if (idmis) good = false;
      // a blank group right after four '\n' follows a group that already ended the records
      // (fastq.go:143-163 and fastq_record's DONTCARE rule): nothing to validate there
      const bool dontcare = known && !good && e0 == s0 && r[s0 - 1] == '\n' && r[s0 - 2] == '\n' &&
                            r[s0 - 3] == '\n' && r[s0 - 4] == '\n';
      if (!act) continue;
      fq_put(S, t, j, L, (uint16_t)(s0 | (good ? 0u : FQ_UNCERT)));
      if (kSpans && good) {  // the record's inner line ends for the filters' spans (0xFFFF: trim the ID globally)
        uint16_t *ln = p.fq_lines + (u64)t * (3 * RCAP) + 3 * L;
        ln[0] = (uint16_t)(idclean ? (e0 | ((crs & 1u) << 15)) : 0xFFFFu);
        ln[1] = (uint16_t)(e1 | ((crs & 2u) << 14));
        ln[2] = (uint16_t)(e2 | ((crs & 4u) << 13));
      }
      if (L + 1 == nrec && known) fq_put(S, t, j, nrec, (uint16_t)(e3 + 1));  // the end of the tile's last record
      if (!good && !dontcare) {  // anything but a certified record: k_fixup validates it from global memory
        const u32 slot = atomicAdd(&S.ndefer, 1u);
        if (slot < (u32)MAX_DEFER) {
          u32 *tdef = kargs()->tile_words + (u64)t * (2 * MAX_DEFER);  // (fq_defer)
          tdef[slot] = L; tdef[MAX_DEFER + slot] = s0;
        } else {
          S.slow = 1;
        }
      }
    }
  }
  __builtin_amdgcn_s_setprio(0);
  TILES_STAMP(3);
  lds_barrier();  // S.ndefer / S.slow / S.line final; the slot and the newline arrays are reused next
  TILES_STAMP(4);
  const u64 word = fq_word(T, gi0, nrec, slow || S.slow, S.ndefer < (u32)MAX_DEFER ? S.ndefer : (u32)MAX_DEFER);
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  {
    // the batch's lines and words leave together after its last tile, from wave 0 (the next
    // batch writes slot 0 only after two more barriers); the lines are read once, by k_fq_place:
    // non-temporal.  (A slow or empty tile's line is never read.)
    if (ptid == 0) S.words[j] = word;
    if (flush && pwid == 0) {
      const KArgs k = kargs();
      uint16_t *lines = reinterpret_cast<uint16_t *>(k->tile_stage);
      u64 *aggs = k->tile_agg;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const u64 t0 = t - j;
      for (u32 c = (u32)lane; c < (j + 1) * (FQ_LINE_E / 8); c += 64) {
        const v4u v = *reinterpret_cast<const v4u *>(&S.line[0][0] + 8 * c);
        __builtin_nontemporal_store(v, (__attribute__((address_space(1))) v4u *)(lines + t0 * FQ_LINE_E + 8 * c));
      }
      if ((u32)lane * 2 < j + 1) {  // the words, 16 bytes per lane (a last odd word alone)
        if ((u32)lane * 2 + 1 < j + 1) {
          const v4u v = *reinterpret_cast<const v4u *>(&S.words[2 * lane]);
          *(__attribute__((address_space(1))) v4u *)(aggs + t0 + 2 * lane) = v;
        } else {
          aggs[t0 + 2 * lane] = S.words[2 * lane];
        }
      }
    }
  }
  TILES_STAMP(5);
#undef TILES_STAMP
}

// Persistent grid-stride over batches of tiles, one LDS slot per workgroup (each tile is staged,
// certified and stored before the next is DMA'd; 7 workgroups per CU keep the DMA busy); no waits
// on other workgroups, so the grid need not be co-resident.
#ifndef SIDX_TILES_WGS
// 7: 21.2 KiB of LDS.  8 per CU needs bursts of 4 tiles (SIDX_FQ_BLK=4: 19.6 KiB) and 64 VGPRs, which the
// compiler meets -- but at eight waves per SIMD it allots 80 SGPRs, not 102, and spills 8 again; with those
// spills the arm ran 0.2-2.5 % faster than 7 per CU (DESIGN.md §3 "Registers of the tile loop"): not adopted
// before the loop is spill-free there too (tests/test_tile_kernel_resources.py holds the product's budget)
#define SIDX_TILES_WGS 7
#endif
template <bool kSpans>
__global__ __launch_bounds__(SNT, SIDX_TILES_WGS) void k_fq_tiles(const SlabParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[SSLOT];
  __shared__ TilesSmem S;
  if (gated_off(p)) return;  // format speculation failed: the host re-runs with the detected format
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  u64 tacc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  u64 *tacc = (tmg(p) && (tid == 0 || tid == 64)) ? tacc_ : nullptr;
  u64 ntl = 0;
  // Claims of up to 32 consecutive tiles taken in file order (a tile's halo, the first KiB of the
  // next tile, is read again by the same workgroup through its own L2 except at a claim's end).
  // Where the workgroups' concurrent streams sit in the input decides how fast they run together:
  // in one process over the C2 input (profiles/r06/calls/j/ab_fq_rr*.json, every table hashed and
  // equal) batches of 32 dealt round-robin ran 1.834-2.034 ms where a contiguous block of 368
  // tiles per workgroup (round 6 before) ran 1.987-2.118, faster on each of eight input copies
  // over three boxes; batches of 8, 16, 24, 48 or 64, or a last round split evenly, all ran slower
  // than 32.  The claims keep that order and hand it out by a counter (claim_loop): no workgroup
  // is left with a twelfth batch while others have finished their eleventh, and one that falls
  // behind takes fewer (DESIGN.md §3 "Tile order").
  claim_loop(S.pad, tid, [&](u32 t, const ClaimRange &r, const ClaimBytes &cb) {
    const u32 j = (t - r.tb) & (FQ_BLK - 1);  // (bursts start at even tiles: the words leave 16 bytes per lane)
    tiles_iter<kSpans>(p, cb, t - r.tb, S, raw, t, tid, lane, wid, tacc, j, j == FQ_BLK - 1 || t + 1 == r.te);
    ++ntl;
  });
  if (tacc) {  // per workgroup: wave 0's phases in slots 0-5, wave 1's in the next 9-slot record
    u64 *o = tmg(p) + ((u64)blockIdx.x * 2 + (tid ? 1 : 0)) * 9;
    for (int i = 0; i < 8; ++i) o[i] = tacc[i];
    o[8] = ntl;
  }
}

// ====================================================================================
// Line index tile pass (line.go:37-45 + index/line.go:33-85, single-slab builds): every '\n'
// ends a row, so a tile needs only its line-number base (scan of the tile counts) and the
// last '\n' before it (a max scan).  k_line_tiles reads the input once: per tile the count,
// the last '\n' and the tile-relative '\n' positions (u16, up to LCAP per tile); k_line_place
// writes the rows (one wave per tile; a tile with more than LCAP lines -- lines under 16 B on
// average -- is rescanned from global memory); k_line_final the last row (the bytes after the
// last '\n', possibly empty: Create always emits it).
// ====================================================================================
constexpr u32 LCAP = TILE / 16;
// Where a tile's positions go: each workgroup of the persistent grid appends its tiles' position
// arrays back to back (16-byte aligned) into its own region of the stage buffer, so the stores of
// consecutive tiles fill whole cache lines; tile_agg[t] = count | the array's offset (16-byte
// units) << 32.  (Fixed 2 KiB slots per tile left a partial line per tile: ablating the stores
// took 0.23-0.37 ms off the kernel, profiles/r04/ab_line_tiles_ablations.txt.)  The region of the
// workgroup whose first tile is t0 starts where t0's would in tile order, t0 * q + min(t0, r)
// tiles in (ntiles = q G + r), and holds LCAP entries per tile it processes.
constexpr u64 LOFF_SHIFT = 32, LCOUNT = (1ull << LOFF_SHIFT) - 1;
#ifndef SIDX_LINE_WGS
#define SIDX_LINE_WGS 7  // workgroups per CU (the slot holds no halo: up to 9 fit the LDS)
#endif
__global__ __launch_bounds__(SNT, SIDX_LINE_WGS) void k_line_tiles(const SlabParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[FRONT + TILE];
  __shared__ __attribute__((aligned(16))) uint16_t sp[LCAP];  // the tile's '\n' positions, stored out whole
  __shared__ u32 wtot[SNW], wlast[SNW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const u64 G = p.pgrid;
  u64 t = first_tile(blockIdx.x, G);
  uint4 *stage16 = reinterpret_cast<uint4 *>(p.tile_stage);
  u64 wofs = (t * (p.ntiles / G) + (t < p.ntiles % G ? t : p.ntiles % G)) * (LCAP / 8);  // 16-byte units
  // A tile's stores leave after the next tile's DMA is issued: vmcnt counts a wave's stores as
  // well as its loads, in issue order, so stores issued before the DMA would be waited for with it
  // (1.768 against 1.778 ms with the stores first, on each of 4 input copies, profiles/r05/calls/r05n)
  u64 pt = ~0ull, pword = 0, ppcnt = 0, pwofs = 0;
  u32 pT = 0;
  auto flush_pending = [&]() -> u32 {  // this wave's store instructions (uniform per wave)
    if (pt == ~0ull) return 0u;
    u32 n = 0;
    if (wid == 0) {
      if (tid == 0) {
        p.tile_agg[pt] = pword;
        p.pcnt[pt] = ppcnt;
      }
      n = 2;
    }
    if (pT <= LCAP && (u32)wid * 512u < pT) {  // (lanes tid * 8 < pT)
      if ((u32)tid * 8 < pT) {
        typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
        const uint4 x = *reinterpret_cast<const uint4 *>(&sp[8 * tid]);
        *reinterpret_cast<v4u_t *>(stage16 + pwofs + (u64)tid) = (v4u_t){x.x, x.y, x.z, x.w};
      }
      ++n;
    }
    pt = ~0ull;
    return n;
  };
  for (; t < p.ntiles; t += G) {
    __builtin_amdgcn_s_setprio(3);
    stage_tile<false>(p, t, (u32)(size_t)(lds_u8 *)raw, wid, lane);
    __builtin_amdgcn_s_setprio(0);
    {  // a wave reads only the bytes it staged: wait for its DMA, not for the stores behind it
      const u32 nst = flush_pending();
      if (nst == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (nst == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      else if (nst == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    }
    const u64 tlo = t * TILE;
    const u32 tlen = (u32)(((tlo + TILE < p.n) ? tlo + TILE : p.n) - tlo);
    u64 m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32 cj = ((u32)j + ((u32)tid >> 2)) & 3u;
      m |= (u64)eq16x(*reinterpret_cast<const uint4 *>(raw + FRONT + tid * 64 + 16 * cj), '\n') << (16 * cj);
    }
    if (eq_suspect(m)) {  // "\n\v" inside a dword: the exact mask
      m = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) m |= (u64)eq16(*reinterpret_cast<const uint4 *>(raw + FRONT + tid * 64 + 16 * j), '\n') << (16 * j);
    }
    const u32 rl = tlen > (u32)tid * 64 ? tlen - (u32)tid * 64 : 0u;
    m &= lowmask(rl);  // bytes past the slab end were zero-filled or are not this tile's
    tail_bytes(p, tlo, tlen, tid, [&](uint8_t c, u32 bit) { m |= (u64)(c == '\n') << bit; });
    const u32 c = popc64(m);
    const u32 incl = wave_scan_add(c);
    const u32 last = m ? (u32)tid * 64 + 64 - clz64(m) : 0u;  // tile-relative '\n' + 1
    const u64 lb = __ballot(m != 0);
    const u32 lmx = lb ? (u32)__builtin_amdgcn_readlane((int)last, 63 - (int)clz64(lb)) : 0u;  // the wave's last
    if (lane == 63) { wtot[wid] = incl; wlast[wid] = lmx; }
    lds_barrier();
    u32 wpre = 0, T = 0, L = 0;
#pragma unroll
    for (int w = 0; w < SNW; ++w) {
      const u32 x = wtot[w];
      if (w < wid) wpre += x;
      T += x;
      L = L > wlast[w] ? L : wlast[w];
    }
    // the positions go through LDS and leave as whole 16-byte stores (scattered 2-byte global
    // stores cost several times their bytes next to the stream); raw is not read past the
    // barrier above, wtot / sp are rewritten only after the next tile's first barrier
    if (T <= LCAP) {
      u32 o = wpre + incl - c;
      u64 mm = m;
      while (mm) {
        sp[o++] = (uint16_t)((u32)tid * 64 + ctz64(mm));
        mm &= mm - 1;
      }
    }
    pt = t;
    pword = (u64)T | (wofs << LOFF_SHIFT);
    ppcnt = L ? tlo + L : (u64)0;  // last '\n' + 1 (absolute), 0: none in the tile
    pwofs = wofs;
    pT = T;
    lds_barrier();
    if (T <= LCAP) wofs += (T + 7) / 8;
  }
  (void)flush_pending();  // the last tile's
}

// The rows of the '\n's in [a, a + 64 * 64) of the tile (wave; lanes take 64-byte words in
// order): line k ends at its '\n', starts after the previous one (`carry` = previous '\n' + 1
// before the range).  Returns the new carry and advances k.
__device__ u64 line_rows_wave(const SlabParams &p, u64 a, u64 hi, u64 carry, u64 &k, int lane) {
  const u64 w = a + 64ull * (u64)lane;
  u64 m = 0;
  if (w < hi) {
    const u64 lim = hi - w < 64 ? hi - w : 64;
    if (lim == 64) {
#pragma unroll
      for (int j = 0; j < 4; ++j) m |= (u64)eq16(load16(p.data + w + 16 * j), '\n') << (16 * j);
    } else {
      for (u64 i = 0; i < lim; ++i) m |= (u64)(p.data[w + i] == '\n') << i;
    }
  }
  const u32 c = popc64(m);
  const u32 incl = wave_scan_add(c);
  const u64 lst = m ? w + 64 - clz64(m) : 0;
  u64 pm = lst;
  for (int d = 1; d < 64; d <<= 1) {
    const u64 y = __shfl_up(pm, d, 64);
    if (lane >= d) pm = pm > y ? pm : y;
  }
  u64 before = __shfl_up(pm, 1, 64);
  if (lane == 0) before = 0;
  u64 start = before > carry ? before : carry;
  u64 kk = k + incl - c;
  while (m) {
    const u64 pos = w + ctz64(m);
    m &= m - 1;
    put_row(p, kk++, start, pos + 1 - start);
    start = pos + 1;
  }
  const u64 tot = (u64)__shfl((int)incl, 63, 64);
  const u64 newc = __shfl(pm, 63, 64);
  k += tot;
  return newc > carry ? newc : carry;
}

// k_line_place: 32 consecutive tiles per workgroup (round 3: one wave per tile, two dependent
// global round trips per wave).  Wave 0 reads the tiles' counts, row bases and carried line
// starts and scans the rows and 16-byte chunks of '\n' positions of the tiles that kept them;
// all lanes stage those chunks in LDS, all in flight together; thread r then writes row r of the
// workgroup's run (its tile by a two-level search of the row prefixes), so the row stores are
// 4 KiB per instruction.  Dense tiles (more than LCAP lines) are rescanned from global memory,
// one wave each; a batch whose positions do not fit LPLACE_ECAP entries places its tiles one
// per wave from global memory.
// SAM (F == F_SAM, k_sam_tiles): the staged positions are the tile's terminator '\n's, the
// first one possibly not a terminator (settled by k_sam_resolve: tile_words bit 30); rows end at
// terminators, the row base is the SamMonoid count before the tile, dense tiles re-run two-pass.
constexpr int LPLACE_TILES = 32;
constexpr u32 LPLACE_ECAP = 12288;  // u16 '\n' positions staged per workgroup (24 KiB)
constexpr u32 SAM_HASNL = 1u << 31, SAM_FIRST_TERM = 1u << 30, SAM_DMASK = SAM_FIRST_TERM - 1;
template <int F>
__global__ __launch_bounds__(256) void k_line_place(const SlabParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t ent[LPLACE_ECAP];
  __shared__ __attribute__((aligned(16))) uint16_t sR[LPLACE_TILES + 8];  // first row of each tile in the run
  __shared__ __attribute__((aligned(16))) uint16_t sC[8];                 // sR[8 j]
  __shared__ u32 sE[LPLACE_TILES + 1];
  __shared__ u64 sB[LPLACE_TILES], sCar[LPLACE_TILES];
  __shared__ uint8_t sO[LPLACE_TILES];  // SAM: 1 when the tile's first staged '\n' is not a terminator
  __shared__ u64 sOff[LPLACE_TILES];    // the tile's position array in the stage buffer (16-byte units)
  __shared__ u32 sDense, sTot;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint16_t *stage = reinterpret_cast<const uint16_t *>(p.tile_stage);
  for (u64 t0 = (u64)blockIdx.x * LPLACE_TILES; t0 < p.ntiles; t0 += (u64)gridDim.x * LPLACE_TILES) {
    if (wid == 0) {
      const u64 t = t0 + (u64)lane;
      const bool valid = lane < LPLACE_TILES && t < p.ntiles;
      u32 rows = 0, chunks = 0;
      bool dense = false;
      if (valid && F == F_SAM) {
        const u32 w = p.tile_words[t], D = w & SAM_DMASK;
        const u32 o = ((w & SAM_HASNL) && !(w & SAM_FIRST_TERM)) ? 1u : 0u;
        sB[lane] = SamMonoid::apply(p.state_in, p.tile_excl[t]) >> 2;
        sCar[lane] = p.ppre[t];
        sO[lane] = (uint8_t)o;
        sOff[lane] = t * (LCAP / 8);  // (k_sam_tiles: one fixed slot per tile)
        if (D <= LCAP) {  // (dense tiles: the build re-runs two-pass, k_sam_tiles flagged it)
          rows = D - o;
          chunks = (D + 7) / 8;
        }
      } else if (valid) {
        const u64 w = p.tile_agg[t], T = w & LCOUNT;
        sOff[lane] = w >> LOFF_SHIFT;
        // row k ends at '\n' number k (rows before the slab: state_in); a slab after the first
        // drops the row open at its start through row_base (put_row)
        sB[lane] = p.state_in + p.tile_excl[t];
        sCar[lane] = p.ppre[t];
        sO[lane] = 0;
        dense = T > LCAP;
        rows = dense ? 0u : (u32)T;
        chunks = (rows + 7) / 8;
      }
      const u32 ri = wave_scan_add(rows), ci = wave_scan_add(chunks);
      const u64 db = __ballot(dense);
      if (lane <= LPLACE_TILES) {
        sR[lane] = (uint16_t)(ri - rows);
        sE[lane] = 8u * (ci - chunks);
        if ((lane & 7) == 0 && lane < LPLACE_TILES) sC[lane >> 3] = (uint16_t)(ri - rows);
      }
      if (lane == 0) sDense = (u32)db;
      if (lane == LPLACE_TILES - 1) sTot = ri;
    }
    __syncthreads();
    const u32 R = sTot, E = sE[LPLACE_TILES];
    if (E <= LPLACE_ECAP) {
      // 8 lanes per tile: chunks c, c + 8, ... of its positions, two loads in flight per step
      const int k = tid >> 3;
      const u32 e0 = sE[k], nch = (sE[k + 1] - e0) >> 3;
      const uint4 *src = reinterpret_cast<const uint4 *>(stage) + sOff[k];
      u32 c = (u32)(tid & 7);
      for (; c + 8 < nch; c += 16) {
        const uint4 a = src[c], b = src[c + 8];
        *reinterpret_cast<uint4 *>(&ent[e0 + 8 * c]) = a;
        *reinterpret_cast<uint4 *>(&ent[e0 + 8 * (c + 8)]) = b;
      }
      if (c < nch) *reinterpret_cast<uint4 *>(&ent[e0 + 8 * c]) = src[c];
      __syncthreads();
      const uint2 cw = *reinterpret_cast<const uint2 *>(sC);
      const u32 c1 = cw.x >> 16, c2 = cw.y & 0xFFFFu, c3 = cw.y >> 16;
      for (u32 r = (u32)tid; r < R; r += 256) {
        const u32 g = (c1 <= r ? 1u : 0u) + (c2 <= r ? 1u : 0u) + (c3 <= r ? 1u : 0u);
        const uint4 fw = *reinterpret_cast<const uint4 *>(&sR[8 * g]);
        const u32 fv[8] = {fw.x & 0xFFFFu, fw.x >> 16, fw.y & 0xFFFFu, fw.y >> 16,
                           fw.z & 0xFFFFu, fw.z >> 16, fw.w & 0xFFFFu, fw.w >> 16};
        u32 kk = 8 * g;
#pragma unroll
        for (int j = 1; j < 8; ++j) kk += (8 * g + (u32)j < (u32)LPLACE_TILES && fv[j] <= r) ? 1u : 0u;
        const u32 L = r - (u32)sR[kk];
        const u32 e = sE[kk] + (u32)sO[kk] + L;
        const u64 tlo = (t0 + kk) * TILE;
        const u32 pos = ent[e];
        const u64 start = L ? tlo + ent[e - 1] + 1 : sCar[kk];
        put_row(p, sB[kk] + L, start, tlo + pos + 1 - start);
      }
    } else {
      for (int k = wid; k < LPLACE_TILES; k += 4) {
        const u32 T = (u32)sR[k + 1] - (u32)sR[k];
        if (!T) continue;
        const uint16_t *st = stage + sOff[k] * 8 + sO[k];
        const u64 tlo = (t0 + k) * TILE;
        for (u32 L = (u32)lane; L < T; L += 64) {
          const u64 start = L ? tlo + st[L - 1] + 1 : sCar[k];
          put_row(p, sB[k] + L, start, tlo + st[L] + 1 - start);
        }
      }
    }
    // dense tiles: rescanned from global memory, one wave each
    for (u32 dm = F == F_LINE ? sDense : 0u; dm; dm &= dm - 1) {
      const int k = (int)__builtin_ctz(dm);
      if ((k & 3) != wid) continue;
      const u64 tlo = (t0 + k) * TILE;
      const u64 hi = (tlo + TILE < p.n) ? tlo + TILE : p.n;
      u64 kr = sB[k], cr = sCar[k];
      for (u64 a = tlo; a < hi; a += 64 * 64) cr = line_rows_wave(p, a, hi, cr, kr, lane);
    }
    __syncthreads();
  }
}

// ppre = exclusive max scan of pcnt (done by the caller): the last row, after the last '\n'
// (index/line.go:33-85 emits it even when empty).  A slab with a halo closes it at the first
// '\n' of the halo (one wave, 1 KiB per step), else at EOF; a halo that ends neither the row
// nor the file is ST_NEEDMORE.  A slab
// with no '\n' at all holds no row of its own (its bytes belong to the row of an earlier slab).
__global__ void k_line_final(const SlabParams p) {
  const int lane = threadIdx.x & 63;
  if (threadIdx.x >= 64 || blockIdx.x) return;
  const u64 t = p.ntiles - 1;
  const u64 c = p.pcnt[t] > p.ppre[t] ? p.pcnt[t] : p.ppre[t];  // last '\n' + 1 of the slab
  const u64 k = p.state_in + p.tile_excl[t] + (p.tile_agg[t] & LCOUNT);
  if (c == 0 && !p.file_start) return;
  for (u64 c0 = p.n & ~15ull; c0 < p.end; c0 += 1024) {  // a slab with a halo: its first '\n'
    const u64 a = c0 + 16ull * (u64)lane;
    u32 m = 0;
    if (a < p.end) {
      m = eq16((a + 16 <= p.end) ? load16(p.data + a) : load16_partial(p.data, a, p.end), '\n');
      if (a < p.n) m &= ~((1u << (u32)(p.n - a)) - 1u);
    }
    const u64 hb = __ballot(m != 0);
    if (hb) {
      const int L = (int)ctz64(hb);
      const u64 q = c0 + 16ull * (u64)L + (u32)__shfl((int)(m ? (u32)__builtin_ctz(m) : 0u), L, 64);
      if (lane == 0) put_row(p, k, c, q + 1 - c);
      return;
    }
  }
  if (p.eof) {  // the bytes after the last '\n' of the file
    if (lane == 0) put_row(p, k, c, p.end - c);
    return;
  }
  if (lane == 0) g_min64(p.badkey, bad_key(k, (u32)t, ST_NEEDMORE));
}

// ====================================================================================
// SAM tile pass (sam.go:83-98 GetReadOffset, single-slab builds): a record ends at the '\n' of
// a "terminator" line -- longer than the '\n' alone, first byte not '@' -- and the next record
// starts after it; header and blank lines belong to the record that follows them.  One read of
// the input, as the line pass:
//   k_sam_tiles    per tile the SamMonoid aggregate (the two-pass build's tile aggregate), the
//                  tile's first '\n' and every later terminator '\n' (u16, a line that starts in
//                  the tile is classed from LDS), the last of those + 1
//   SamMonoid scan -> each tile's incoming state: terminators before it, open-line class
//   k_sam_resolve  the first '\n' of a tile: a terminator iff the open line is a data line, or
//                  the tile starts a line whose first byte is neither '\n' nor '@'
//   max scan       of the last terminator + 1 -> each tile's first row start
//   k_line_place<F_SAM>, k_sam_final (the bytes after the last terminator, a row when not empty;
//                  else no record: ST_ABSENT, as sam_record at EOF)
// A tile with more than LCAP '\n's (lines under 16 bytes on average) makes the build re-run
// two-pass (counters[3] bit 0, as a k_fixup overflow).
// ====================================================================================
__global__ __launch_bounds__(SNT, SIDX_LINE_WGS) void k_sam_tiles(const SlabParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[FRONT + TILE];
  __shared__ __attribute__((aligned(16))) uint16_t sp[LCAP];
  __shared__ u32 wlast[SNW], wtot[SNW], wkeep[SNW];
  __shared__ u64 wagg[SNW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const u64 G = p.pgrid;
  u64 t = first_tile(blockIdx.x, G);
  uint16_t *stage = reinterpret_cast<uint16_t *>(p.tile_stage);
  for (; t < p.ntiles; t += G) {
    __builtin_amdgcn_s_setprio(3);
    stage_tile<false>(p, t, (u32)(size_t)(lds_u8 *)raw, wid, lane);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // a wave reads only the bytes it staged
    const u64 tlo = t * TILE;
    const u32 tlen = (u32)(((tlo + TILE < p.n) ? tlo + TILE : p.n) - tlo);
    const uint8_t *b = raw + FRONT;
    u64 m = 0, at = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint4 v = *reinterpret_cast<const uint4 *>(b + tid * 64 + 16 * j);
      m |= (u64)eq16(v, '\n') << (16 * j);
      at |= (u64)eq16(v, '@') << (16 * j);
    }
    const u32 rl = tlen > (u32)tid * 64 ? tlen - (u32)tid * 64 : 0u;
    tail_bytes(p, tlo, tlen, tid, [&](uint8_t c, u32 bit) {
      m |= (u64)(c == '\n') << bit;
      at |= (u64)(c == '@') << bit;
    });
    m &= lowmask(rl);
    at &= lowmask(rl);
    const u32 len = rl < 64 ? rl : 64u;
    const u64 wi = wave_incl_scan<SamMonoid>(SamMonoid::seg(m, at, len), lane);
    // previous '\n' + 1 before this thread's word, inside the tile (0: none)
    const u32 last = m ? (u32)tid * 64 + 64 - clz64(m) : 0u;
    // (not wave_scan_max: next to the SamMonoid scan the DPP form takes 67 VGPRs instead of 60, one
    // workgroup per CU less)
    u32 pm = last;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u32 y = (u32)__shfl_up((int)pm, d, 64);
      if (lane >= d) pm = pm > y ? pm : y;
    }
    u32 before = (u32)__shfl_up((int)pm, 1, 64);
    if (lane == 0) before = 0;
    if (lane == 63) { wlast[wid] = pm; wagg[wid] = wi; }
    lds_barrier();
    for (int w = 0; w < wid; ++w) before = before > wlast[w] ? before : wlast[w];
    // the thread's kept '\n's: the tile's first one (settled later) and every terminator whose
    // line starts in the tile
    u64 keep = 0;
    u32 lk = 0;  // last terminator + 1 (tile-relative), the first '\n' excluded
    {
      u32 pp = before;
      for (u64 mm = m; mm; mm &= mm - 1) {
        const u32 q = (u32)tid * 64 + ctz64(mm);
        if (!pp) {
          keep |= 1ull << (q & 63);
        } else if (pp < q && b[pp] != '@') {
          keep |= 1ull << (q & 63);
          lk = q + 1;
        }
        pp = q + 1;
      }
    }
    const u32 c = popc64(keep);
    const u32 incl = wave_scan_add(c);
    const u64 kb = __ballot(lk != 0);
    const u32 lkw = kb ? (u32)__builtin_amdgcn_readlane((int)lk, 63 - (int)clz64(kb)) : 0u;
    if (lane == 63) { wtot[wid] = incl; wkeep[wid] = lkw; }
    lds_barrier();
    u32 wpre = 0, D = 0, LK = 0, anynl = 0;
    u64 agg = SamMonoid::identity();
#pragma unroll
    for (int w = 0; w < SNW; ++w) {
      const u32 x = wtot[w];
      if (w < wid) wpre += x;
      D += x;
      LK = LK > wkeep[w] ? LK : wkeep[w];
      anynl |= wlast[w];
      agg = SamMonoid::combine(agg, wagg[w]);
    }
    if (D <= LCAP) {
      u32 o = wpre + incl - c;
      for (u64 kk = keep; kk; kk &= kk - 1) sp[o++] = (uint16_t)((u32)tid * 64 + ctz64(kk));
    }
    if (tid == 0) {
      p.tile_agg[t] = agg;
      p.pcnt[t] = LK ? tlo + LK : 0;
      p.tile_words[t] = D | (anynl ? SAM_HASNL : 0u);
      if (D > LCAP) atomicOr(&p.counters[3], 1u);  // dense tile: re-run two-pass
    }
    lds_barrier();
    if (D <= LCAP && (u32)tid * 8 < D)
      reinterpret_cast<uint4 *>(stage + t * LCAP)[tid] = *reinterpret_cast<const uint4 *>(&sp[8 * tid]);
  }
}

// The first '\n' of every tile: a terminator iff the line open at the tile start is a data line
// (SamMonoid state 1), or the tile starts a line (state 0) whose first byte is neither '\n' nor
// '@' (the monoid's dF).  A tile whose only terminator it is takes its end as its last one.
__global__ void k_sam_resolve(const SlabParams p) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.ntiles) return;
  const u32 w = p.tile_words[t];
  if (!(w & SAM_HASNL) || (w & SAM_DMASK) > LCAP) return;
  const u32 st = (u32)(SamMonoid::apply(p.state_in, p.tile_excl[t]) & 3);
  const u64 tlo = t * TILE;
  const u32 b0 = p.data[tlo];
  if (!(st == 1 || (st == 0 && b0 != '\n' && b0 != '@'))) return;
  p.tile_words[t] = w | SAM_FIRST_TERM;
  if (!p.pcnt[t]) p.pcnt[t] = tlo + reinterpret_cast<const uint16_t *>(p.tile_stage)[t * LCAP] + 1;
}

// The record after the last terminator: the rest of the file, or none when nothing is left
// (sam_record at EOF: ST_ABSENT, so the count is the number of terminators).
__global__ void k_sam_final(const SlabParams p) {
  if (threadIdx.x || blockIdx.x) return;
  const u64 t = p.ntiles - 1;
  const u64 c = p.pcnt[t] > p.ppre[t] ? p.pcnt[t] : p.ppre[t];  // last terminator + 1 (0: none)
  const u64 k = SamMonoid::apply(p.state_in, SamMonoid::combine(p.tile_excl[t], p.tile_agg[t])) >> 2;
  if (p.end > c) put_row(p, k, c, p.end - c);
  else g_min64(p.badkey, bad_key(k, (u32)t, ST_ABSENT));
}

// k_fq_place: 64 consecutive tiles per workgroup, in three steps with one global round trip
// each (round 3 placed a tile per wave at a time, two dependent u16 loads before every row
// store: 16 serial load latencies per wave, 0.17 ms at C2).
//  1. wave 0, lane k = tile t0 + k: the tile's word and scan prefix decide it -- its rows when
//     the phase read off the tile was right, else the whole tile to k_fixup; a wave scan of the
//     placed tiles' record counts gives each tile its first row in the workgroup's run, a scan of
//     their 16-byte chunks of u16 starts its place in LDS;
//  2. every lane loads 16-byte chunks of the tiles' start arrays into LDS, all in flight together;
//  3. thread r writes row r of the workgroup's run (its tile by a two-level search of the row
//     prefixes: one 16-byte LDS read of every 8th prefix, one of the 8 in that group), so each
//     store instruction writes 4 KiB of consecutive rows.
// A batch whose starts do not fit PLACE_ECAP entries (records under ~140 bytes) places its tiles
// one per wave from global memory instead.
constexpr int PLACE_TILES = 64;
constexpr u32 PLACE_ECAP = 8192;  // u16 starts staged per workgroup (16 KiB)
__global__ __launch_bounds__(256) void k_fq_place(const SlabParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t ent[PLACE_ECAP];
  __shared__ __attribute__((aligned(16))) uint16_t sR[PLACE_TILES + 8];  // first row of each tile (+ total)
  __shared__ __attribute__((aligned(16))) uint16_t sC[8];                // sR[8 j]
  __shared__ u32 sE[PLACE_TILES + 1];                                    // first LDS entry of each tile
  __shared__ u64 sG[PLACE_TILES];                                        // global number of local record 0
  if (gated_off(p)) return;  // format speculation failed: the host re-runs with the detected format
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (u64 t0 = (u64)blockIdx.x * PLACE_TILES; t0 < p.ntiles; t0 += (u64)gridDim.x * PLACE_TILES) {
    if (wid == 0) {
      const u64 t = t0 + (u64)lane;
      u32 rows = 0, chunks = 0;
      u64 gbase = 0;
      if (t < p.ntiles) {
        const FqTileWord f = fq_unpack(p, t);
        if (!f.redo) {
          gbase = f.gbase;
          rows = f.nrec;
          // starts 0..nrec (entry nrec: the last record's end): the tile's line, then its overflow
          chunks = rows ? (rows + 8) / 8 : 0u;
          const u32 *tdef = fq_defer(p, t);
          for (u32 i = 0; i < f.nd; ++i) push_fix(p, t * TILE + tdef[MAX_DEFER + i], gbase + tdef[i], (u32)t);
        } else {
          push_fix(p, ~0ull, f.j0, (u32)t);  // whole tile, true rank j0
        }
      }
      const u32 ri = wave_scan_add(rows), ci = wave_scan_add(chunks);
      sR[lane] = (uint16_t)(ri - rows);
      sE[lane] = 8u * (ci - chunks);  // the tile's entry 0 (its chunks staged from there)
      sG[lane] = gbase;
      if ((lane & 7) == 0) sC[lane >> 3] = (uint16_t)(ri - rows);
      if (lane == 63) { sR[PLACE_TILES] = (uint16_t)ri; sE[PLACE_TILES] = 8u * ci; }
    }
    __syncthreads();
    const u32 R = sR[PLACE_TILES], E = sE[PLACE_TILES];
    if (E <= PLACE_ECAP) {
      // step 2: lanes 4 k' .. 4 k' + 3 of wave w stage tile 16 w + k' (chunks c, c + 4, ...)
      const int k = wid * 16 + (lane >> 2);
      const u32 e0 = sE[k], nch = (sE[k + 1] - e0) >> 3;
      const u64 tk = t0 + (u64)k;
      // chunks 0..7: the tile's line; 8..: its overflow slot (two loads in flight per step)
      const uint4 *ln = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p.tile_stage) + tk * FQ_LINE_E);
      const uint4 *ov = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p.tile_stage) + fq_ovf(p, tk)) -
                        FQ_LINE_E / 8;
      u32 c = (u32)(lane & 3);
      for (; c + 4 < nch; c += 8) {
        const uint4 a = c < FQ_LINE_E / 8 ? ln[c] : ov[c], b = c + 4 < FQ_LINE_E / 8 ? ln[c + 4] : ov[c + 4];
        *reinterpret_cast<uint4 *>(&ent[e0 + 8 * c]) = a;
        *reinterpret_cast<uint4 *>(&ent[e0 + 8 * (c + 4)]) = b;
      }
      if (c < nch) *reinterpret_cast<uint4 *>(&ent[e0 + 8 * c]) = c < FQ_LINE_E / 8 ? ln[c] : ov[c];
      __syncthreads();
      // step 3: row r of the run
      const uint4 cw = *reinterpret_cast<const uint4 *>(sC);
      const u32 cv[8] = {cw.x & 0xFFFFu, cw.x >> 16, cw.y & 0xFFFFu, cw.y >> 16,
                         cw.z & 0xFFFFu, cw.z >> 16, cw.w & 0xFFFFu, cw.w >> 16};
      for (u32 r = (u32)tid; r < R; r += 256) {
        u32 g = 0;
#pragma unroll
        for (int j = 1; j < 8; ++j) g += cv[j] <= r ? 1u : 0u;
        const uint4 fw = *reinterpret_cast<const uint4 *>(&sR[8 * g]);
        const u32 fv[8] = {fw.x & 0xFFFFu, fw.x >> 16, fw.y & 0xFFFFu, fw.y >> 16,
                           fw.z & 0xFFFFu, fw.z >> 16, fw.w & 0xFFFFu, fw.w >> 16};
        u32 kk = 8 * g;
#pragma unroll
        for (int j = 1; j < 8; ++j) kk += fv[j] <= r ? 1u : 0u;
        const u32 L = r - (u32)sR[kk];
        const u32 e = sE[kk] + L;
        const u32 rv = ent[e], nx = ent[e + 1];
        if (!(rv & FQ_UNCERT)) put_row(p, sG[kk] + L, (t0 + kk) * TILE + rv, (nx & ~FQ_UNCERT) - rv);
      }
    } else {
      for (int k = wid; k < PLACE_TILES; k += 4) {
        const u32 rows = (u32)sR[k + 1] - (u32)sR[k];
        const u64 tk = t0 + (u64)k;
        for (u32 L = (u32)lane; L < rows; L += 64) {
          const u32 rv = fq_start(p, tk, L);
          if (!(rv & FQ_UNCERT)) put_row(p, sG[k] + L, tk * TILE + rv, (fq_start(p, tk, L + 1) & ~FQ_UNCERT) - rv);
        }
      }
    }
    __syncthreads();
  }
}

// (download filters, sidx_filter.hip) The ID / sequence / quality spans of every record the
// FASTQ tile pass certified, from the line ends it kept (k_fq_tiles<true>: no re-read of the
// section): sidx_filter's layout, 6 u32 per record relative to its start, and the record's output
// length with bit 63 set ("done").  Records it did not certify, IDs whose TrimSpace is more than
// the line end, and whole tiles sent to k_fixup are left to k_fq_spans (their outlen stays 0).
// One wave per tile.
__device__ __forceinline__ u32 ndigits10(u64 v) {
  u32 d = 1;
  u64 q = 10;
#pragma unroll
  for (int k = 1; k < 20; ++k) {
    d += v >= q ? 1u : 0u;
    q *= 10;
  }
  return d;
}
__global__ __launch_bounds__(256) void k_fq_spans_place(const SlabParams p, u32 *spans, u64 *outlen, u64 K, int kind) {
  const int lane = threadIdx.x & 63;
  const u64 nw = (u64)gridDim.x * 4;
  for (u64 t = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); t < p.ntiles; t += nw) {
    const FqTileWord f = fq_unpack(p, t);
    if (f.redo) continue;  // the whole tile went to k_fixup
    const uint16_t *ln = p.fq_lines + t * (3 * RCAP);
    for (u32 L = (u32)lane; L < f.nrec; L += 64) {
      const u64 g = f.gbase + L;
      const u32 rv = fq_start(p, t, L);
      if (g < p.row_base || g - p.row_base >= K || (rv & FQ_UNCERT)) continue;
      const u32 x0 = ln[3 * L];
      if (x0 == 0xFFFFu) continue;
      const u32 x1 = ln[3 * L + 1], x2 = ln[3 * L + 2], nx = fq_start(p, t, L + 1) & ~FQ_UNCERT;
      const u32 e0 = x0 & 0x7FFFu, e1 = x1 & 0x7FFFu, e2 = x2 & 0x7FFFu, e3 = nx - 1;
      const u32 z0 = e0 - (x0 >> 15), z1 = e1 - (x1 >> 15), z3 = e3 - (x2 >> 15);
      const u32 il = z0 - rv - 1, sl = z1 - e0 - 1, ql = z3 - e2 - 1;
      const u64 i = g - p.row_base;
      u32 *sp = spans + 6 * i;
      sp[0] = 1u; sp[1] = il;
      sp[2] = e0 + 1 - rv; sp[3] = sl;
      sp[4] = e2 + 1 - rv; sp[5] = ql;
      const u64 len = kind == 1 ? (u64)il + sl + 3 : (u64)ndigits10(i + 1) + sl + ql + 6;
      outlen[i] = len | (1ull << 63);
    }
  }
}

// Record starting at s validated from global memory by the whole wave.
__device__ __forceinline__ void fix_record(const SlabParams &p, u64 s, u64 g, u32 tile, int lane) {
  WaveAcc wa;
  wa.g = p.data; wa.end = p.end; wa.eof = p.eof; wa.lane = lane; wa.front = p.front;
  u64 len = 0, epos = 0, elen = 0;
  const u32 st = run_record_cold<F_FASTQ>(wa, s, 0, len, epos, elen);
  if (lane == 0) {
    if (st == ST_OK) put_row(p, g, s, len);
    else atomicMin(p.badkey, bad_key(g, tile, st));
  }
}

// k_fixup: the records and tiles k_fq_tiles / k_fq_place queued, one wave per item.  A tile is re-indexed
// with its true newline rank j0: every '\n' of rank 3 mod 4 starts a record.  Its last workgroup to
// finish (a ticket in counters[7]) then runs k_finalize's body: one launch less per build.
struct DevResult;
__device__ __forceinline__ void finalize_body(const SlabParams &p, int fmt, DevResult *res);
__device__ __forceinline__ void last_block_finalize(const SlabParams &p, int fmt, DevResult *res) {
  // every storing wave's stores (rows, FASTA detail slots) complete, then one release per
  // workgroup before its ticket; the last workgroup acquires (MI355X_MICROARCH.md, valid forms)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const u32 k = __hip_atomic_fetch_add(&p.counters[7], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      finalize_body(p, fmt, res);
    }
  }
}
__global__ __launch_bounds__(256) void k_fixup(const SlabParams p, DevResult *res) {
  if (gated_off(p)) {
    if (res) last_block_finalize(p, F_FASTQ, res);
    return;
  }
  const int lane = threadIdx.x & 63;
  const u32 nw = gridDim.x * (blockDim.x / 64);
  const u32 wv = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const u32 n = p.counters[2] < p.fixcap ? p.counters[2] : (u32)p.fixcap;
  for (u32 i = wv; i < n; i += nw) {
    const FixRec f = reinterpret_cast<const FixRec *>(p.fix)[i];
    if (f.start != ~0ull) {
      fix_record(p, f.start, f.g, f.tile, lane);
      continue;
    }
    const u32 tile = f.tile;
    const u64 tlo = (u64)tile * TILE;
    const u64 thi = (tlo + TILE < p.n) ? tlo + TILE : p.n;
    if (p.file_start && tile == 0) fix_record(p, 0, 0, tile, lane);
    u64 rank = f.g;
    for (u64 b = tlo; b < thi; b += 1024) {
      const u64 a = b + (u64)lane * 16;
      u32 m = 0;
      if (a < thi) m = eq16((a + 16 <= thi) ? load16(p.data + a) : load16_partial(p.data, a, thi), '\n');
      const u32 c = __popc(m);
      const u32 incl = wave_scan_add(c);
      u64 cand = __ballot(m != 0);
      while (cand) {
        const int L = (int)ctz64(cand);
        cand &= cand - 1;
        u32 mL = (u32)__shfl((int)m, L, 64);
        u64 rr = rank + (u32)__shfl((int)(incl - c), L, 64);
        while (mL) {
          const u32 bit = (u32)__builtin_ctz(mL);
          mL &= mL - 1;
          if ((rr & 3) == 3) fix_record(p, b + 16 * (u64)L + bit + 1, (rr + 1) >> 2, tile, lane);
          ++rr;
        }
      }
      rank += (u32)__shfl((int)incl, 63, 64);
    }
  }
  if (res) last_block_finalize(p, F_FASTQ, res);
}

// ====================================================================================
// FASTA tile pass: k_fa_tiles -> scan of the tile aggregates (FastaMonoid) -> k_fa_place ->
// k_fa_fixup.  The input is read once.
//
// fasta.go:93-140 restated per tile: a '>' is a record boundary iff a '\n' occurred since the
// previous '>' (the FastaMonoid).  Inside a tile every '>' but possibly the first is decided
// locally; the tile's first '>' with no '\n' before it in the tile is "conditional" -- a
// boundary iff the tile is entered armed, known after the scan.  The candidates (the
// boundaries plus the conditional '>') go to a provisional table as tile-relative positions.
//
// Validation is owned by the END of a record: the piece that closes a record is the bytes
// since the previous '>' (fasta.go:111-121, TrimSpace must leave a '\n' inside), so the tile
// holding the closing '>' checks it from LDS.  A piece that starts in an earlier tile is
// certified from its part in this tile when that part alone shows a '\n' between two ASCII
// non-space bytes; anything undecidable here (such pieces otherwise, non-ASCII bytes at a
// trimmed edge, the conditional '>') goes to k_fa_fixup, which re-checks it from global
// memory.  Rows are owned by the START of a record: k_fa_place writes the row of the record
// opened by each boundary, its end being the next candidate of the tile or, for the tile's
// last boundary, the first boundary of a later tile (read off the tile words).
// ====================================================================================
constexpr u32 FA_OK = 0, FA_INV = 1, FA_DEFER = 2, FA_SKIP = 3;  // SKIP: owned by the previous slab
// Measured choices (round 5, one-process A/B tables under profiles/r05/calls/): the tile
// certificate's '\n' lookup over two mask words in one LDS round; fa_check's fast path looks at
// FA_NLW = 2 mask words (2.12 -> 1.99 ms, r05fa); a word's candidate count by carries instead of a
// loop over its '>' (1.976 -> 1.929 and 2.050 -> 2.021 ms on two input copies, r05fg).  Dropped:
// the tile's stores issued after the next tile's DMA (2.26 against 2.12 ms, r05n).
constexpr int FA_NLW = 2;
constexpr u32 FA_NONE = ~0u;
constexpr int FAW = 8;  // rare tile words: -, -, -, -, finv, inv_lo (a tile with an invalid piece), eof_st, eof_lo (the last tile)
// The per-tile word (tile_agg[t]): the FastaMonoid aggregate in bits 0-17 (what the scan folds),
// the candidate count, slow / conditional-first flags, the first conditional and the first
// definite boundary (15 bits each, 0x7FFF: none) and whether tw[4..5] hold an invalid piece --
// one u64 store per tile instead of a 32-byte record (the k_fq_tiles note on stores).
constexpr u64 FAW_AMASK = 0x3FFFF;
__device__ __forceinline__ u64 fa_word(u64 A, u32 ncand, bool slow, u32 delta, u32 fc, u32 fd, bool hasinv,
                                       bool tcert) {
  const u32 nc = ncand < 0xFFFu ? ncand : 0xFFFu;  // more than RCAP means slow anyway
  return (A & FAW_AMASK) | ((u64)nc << 18) | ((u64)tcert << 30) | ((u64)slow << 31) | ((u64)(delta & 1u) << 32) |
         ((u64)(fc & 0x7FFFu) << 33) | ((u64)(fd & 0x7FFFu) << 48) | ((u64)hasinv << 63);
}
// bit 30: the piece open at the tile's end (from its last '>', or from before the tile) holds a
// '\n' between two ASCII non-space bytes inside this tile -- whatever the rest of the piece is,
// TrimSpace keeps that '\n' inside, so the piece passes fasta.go:111-121 (the next tile's first
// piece, undecidable from its own part, is then settled without k_fa_fixup)
__device__ __forceinline__ bool fa_w_tcert(u64 w) { return (w >> 30) & 1u; }
__device__ __forceinline__ u32 fa_w_none(u32 x) { return x == 0x7FFFu ? FA_NONE : x; }
__device__ __forceinline__ u32 fa_w_flags(u64 w) { return (u32)((w >> 31) & 1u) | ((u32)((w >> 32) & 1u) << 1); }
__device__ __forceinline__ u32 fa_w_fc(u64 w) { return fa_w_none((u32)(w >> 33) & 0x7FFFu); }
__device__ __forceinline__ u32 fa_w_fd(u64 w) { return fa_w_none((u32)(w >> 48) & 0x7FFFu); }

struct __align__(16) FaSmem {
  u64 mnl[TILE / 64];
  u32 cand[RCAP];  // candidate: tile-relative '>' | (previous '>' + 1, 0: none in the tile) << 14
  u64 wagg[SNW];   // per wave: candidates | conditional << 20
  u32 wlast[SNW];  // per wave: last '>' + 1
  u32 wnl[SNW];    // per wave: last '\n' + 1
  u32 finv, tcert, pad[2];
};
static_assert(TILE <= (1 << 14), "candidate packing: 14-bit positions");

// first '\n' in [a, b) of the tile (mask words), b if none
__device__ __forceinline__ u32 fa_find_nl(const u64 *mnl, u32 a, u32 b) {
  if (a >= b) return b;
  u32 w = a >> 6;
  const u32 wl = (b - 1) >> 6;
  u64 m = mnl[w] & (~0ull << (a & 63));
  for (;;) {
    if (m) {
      const u32 q = (w << 6) + ctz64(m);
      return q < b ? q : b;
    }
    if (w == wl) return b;
    m = mnl[++w];
  }
}

// fasta.go:111-121 on the piece [lo, g) of the tile: TrimSpace leaves a '\n' inside.  ASCII
// edges only; an edge byte >= 0x80 (unicode.IsSpace may trim it) is left to the fixup.
// `part`: the piece starts before the tile, [lo, g) is only its tail -- then a '\n' between
// two ASCII non-space bytes certifies it and anything else is undecided.
__device__ __forceinline__ u32 fa_check(const uint8_t *r, const u64 *mnl, u32 lo, u32 g, bool part) {
  // the common piece in one LDS round: its first byte and the byte before its closing "\n>"
  // are printable ASCII (TrimSpace keeps [lo, g - 1)) and the '\n' ending its first line is
  // in the mask word of lo -- that '\n' is then the first one fa_find_nl would return
  if (g >= lo + 3) {
    // the first '\n' from lo within FA_NLW mask words, all read in one LDS round: with one
    // word, a header line running past lo's 64 bytes (about half of C3's records) took the loops
    // below -- 2.12 -> 1.99 ms for k_fa_tiles with two words (profiles/r05/calls/r05fa)
    const u32 c0 = r[lo], c1 = r[g - 1], c2 = r[g - 2];
    const u32 wi = lo >> 6;
    u64 w[FA_NLW];
#pragma unroll
    for (int k = 0; k < FA_NLW; ++k) w[k] = wi + k < (u32)(TILE / 64) ? mnl[wi + k] : 0ull;
    w[0] &= ~0ull << (lo & 63);
    u32 q = ~0u;
#pragma unroll
    for (int k = FA_NLW - 1; k >= 0; --k)
      if (w[k]) q = ((wi + (u32)k) << 6) + ctz64(w[k]);
    if (ascii_nonspace(c0) && c1 == '\n' && ascii_nonspace(c2) && q < g - 1) return FA_OK;
  }
  u32 f = lo;
  while (f < g && ascii_space(r[f])) ++f;
  if (f == g) return part ? FA_DEFER : FA_INV;
  u32 e = g;
  while (ascii_space(r[e - 1])) --e;  // stops at f + 1 at the latest
  if (r[f] >= 0x80 || r[e - 1] >= 0x80) return FA_DEFER;
  if (fa_find_nl(mnl, f, e) < e) return FA_OK;
  return part ? FA_DEFER : FA_INV;
}

__device__ __forceinline__ void fa_iter(const SlabParams &p, const ClaimBytes &cb, u32 rel, FaSmem &S, uint8_t *raw,
                                        u32 t, int tid, int lane, int wid) {
  // (predicates only: addresses use tid / lane; one copy, the kernel has no vector register to spare)
  int ptid = tid;
  asm volatile("" : "+v"(ptid));
  const int plane = ptid & 63;
  const u32 tlen = cb.tlen(rel), llen = cb.llen(rel);
  const uint8_t *tile0 = cb.base + rel * (u32)TILE;
  __builtin_amdgcn_s_setprio(3);  // as k_fq_tiles: DMA issue, then the certification, first
  // the tile alone: no halo, no front
  stage_tile_at<false>(tile0, llen, !tile_nofront(t), (u32)(size_t)(lds_u8 *)raw, wid, lane, plane);
  __builtin_amdgcn_s_setprio(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // a wave classifies only the bytes it staged
  if (ptid == 0) S.finv = FA_NONE;
  if (llen < (u32)TILE && (llen & 3u)) {  // slab end: the partial last dword came back as zeros
    lds_barrier();
    if (ptid == 0) {
      const u32 o = llen & ~15u;
      uint4 v = keep_bytes(*reinterpret_cast<const uint4 *>(raw + FRONT + o), llen - o);
      const auto rs = tile_rsrc_at(tile0, llen);
      patch_tail(v, o, llen, tail_dword(rs, llen));
      *reinterpret_cast<uint4 *>(raw + FRONT + o) = v;
    }
    lds_barrier();
  }
  const uint8_t *r = raw + FRONT;
  // ---- '\n' / '>' mask words, the candidates -----------------------------------------------
  // A '>' at j is a candidate (fasta.go:100-138) iff a '\n' occurred since the previous '>':
  // with pg / pn = the last '>' / '\n' before j (+ 1, 0: none in the tile), iff pn > pg, or
  // pg == 0 (the tile's first '>': a boundary if pn > 0, else conditional on the state the
  // tile is entered in).  Inside a wave, pg and pn come from two max scans; only a wave's first
  // '>' with no '\n' before it in the wave depends on the earlier waves, and is settled after
  // the barrier by a fold over the four wave summaries.
  u64 nl = 0, gt = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u32 cj = ((u32)j + ((u32)tid >> 2)) & 3u;
    const uint4 v = *reinterpret_cast<const uint4 *>(r + tid * 64 + 16 * cj);
    nl |= (u64)eq16x(v, '\n') << (16 * cj);
    gt |= (u64)eq16x(v, '>') << (16 * cj);
  }
  if (eq_suspect(nl) || eq_suspect(gt)) {  // two flags of one kind side by side in a dword ("\n\v", ">?"): exact masks
    nl = gt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint4 v = *reinterpret_cast<const uint4 *>(r + tid * 64 + 16 * j);
      nl |= (u64)eq16(v, '\n') << (16 * j);
      gt |= (u64)eq16(v, '>') << (16 * j);
    }
  }
  const u32 rl0 = tlen > (u32)tid * 64 ? tlen - (u32)tid * 64 : 0u;
  const u32 rl = rl0 < 64 ? rl0 : 64u;
  nl &= lowmask(rl);
  gt &= lowmask(rl);
  S.mnl[tid] = nl;
  const u32 base = (u32)tid * 64;
  const u32 ln = nl ? base + 64 - clz64(nl) : 0u;  // last '\n' + 1
  const u32 lg = gt ? base + 64 - clz64(gt) : 0u;  // last '>' + 1
  const u32 NLi = wave_scan_max(ln), GTi = wave_scan_max(lg);
  // the previous lane's two values by one DPP wave shift (lane 0 reads 0); positions + 1 <= 2^14
  const u32 pk = (u32)__builtin_amdgcn_update_dpp(0, (int)((NLi << 16) | GTi), 0x138, 0xF, 0xF, false);
  const u32 NLx = pk >> 16, GTx = pk & 0xFFFFu;  // before this word, in the wave
  // a '>' is a candidate iff the marker ('>' or '\n') nearest below it is a '\n': one carry per
  // '\n' (and one at bit 0 when the word is entered after a '\n') runs up through the non-marker
  // bits of ~u and lands on the next marker; the wave's first '>' with no marker below it at all
  // is the conditional one
  const u64 u = nl | gt;
  const u32 c = popc64(gt & (~u + (nl << 1) + (NLx > GTx ? 1ull : 0ull)));
  const u32 cond = (GTx == 0 && NLx == 0 && (u & (0ull - u) & gt)) ? 1u : 0u;
  const u32 incl = wave_scan_add(c);
  const bool wcond = __ballot(cond) != 0;
  if (plane == 63) {
    S.wagg[wid] = incl | (wcond ? 1u << 20 : 0u);
    S.wlast[wid] = GTi;
    S.wnl[wid] = NLi;
  }
  lds_barrier();
  // fold of the wave summaries in order: candidates before this wave, its first '>' settled
  u32 PN = 0, PG = 0, cnt = 0, delta = 0, myPG = 0, mybase = 0, mycond = 0;
#pragma unroll
  for (int w = 0; w < SNW; ++w) {
    // uniform values: the fold runs on the scalar unit
    const u32 a = (u32)__builtin_amdgcn_readfirstlane((int)(u32)S.wagg[w]);
    const u32 gw = (u32)__builtin_amdgcn_readfirstlane((int)S.wlast[w]);
    const u32 nw = (u32)__builtin_amdgcn_readfirstlane((int)S.wnl[w]);
    if (w == wid) { myPG = PG; mybase = cnt; }
    u32 cw = 0;
    if (a >> 20) {
      if (PG == 0 && PN == 0) { delta = 1; cw = 1; }  // the tile's first '>', conditional
      else if (PG == 0 || PN > PG) cw = 1;
    }
    if (w == wid) mycond = cw;
    cnt += cw + (a & 0xFFFFFu);
    PN = umax(PN, nw);
    PG = umax(PG, gw);
  }
  const u32 ncand = cnt;
  const u32 alast = PG;
  const u64 A = FastaMonoid::mk(cnt - delta, delta, (PN | PG) == 0 ? 0u : (PN > PG ? 2u : 1u));
  // ---- candidates of this word, in order ----------------------------------------------------
  if (gt) {
    u32 idx = mybase + mycond + incl - c;
    u32 pg = GTx, pga = GTx ? GTx : myPG;  // previous '>' + 1: in the wave / in the tile
    for (u64 m = gt; m;) {
      const u32 j = ctz64(m);
      m &= m - 1;
      const u64 nb = nl & lowmask(j);
      const u32 pn = nb ? base + 64 - clz64(nb) : NLx;
      u32 slot = FA_NONE;
      if (pg == 0 && pn == 0) slot = mycond ? mybase : FA_NONE;
      else if (pg == 0 || pn > pg) slot = idx++;
      if (slot < (u32)RCAP) S.cand[slot] = (base + j) | (pga << 14);
      pg = pga = base + j + 1;
    }
  }
  lds_barrier();
  // ---- validation of the pieces that close at the candidates -------------------------------
  __builtin_amdgcn_s_setprio(2);
  const bool slow = ncand > (u32)RCAP;
  uint16_t *stage = reinterpret_cast<uint16_t *>(p.tile_stage + (u64)t * RCAP);  // position | status << 14
  // A slab after the file's first: its first tile's first boundary (the incoming state is known
  // there) closes the record open at the slab start, which the previous slab owns and checks
  // through its halo; any other piece starting before data[0] is checked as a part (never INV).
  bool fs = false;  // the file's first tile
  u32 skip0 = ~0u;
  if (t == 0) {
    const KArgs k = kargs();
    fs = k->file_start != 0;
    if (!fs) skip0 = (delta && !(k->state_in & 1)) ? 1u : 0u;
  }
  if (!slow) {
    for (u32 i = (u32)tid; i < ncand; i += SNT) {
      const u32 c = S.cand[i];
      const u32 g = c & 0x3FFFu, lo = c >> 14;
      u32 st;
      if (i == skip0) st = FA_SKIP;
      else if (i == 0 && delta) st = FA_DEFER;  // conditional: its piece has no '\n' in this tile
      else st = fa_check(r, S.mnl, lo, g, lo == 0 && !fs);
      stage[i] = (uint16_t)(g | (st << 14));
      if (st == FA_INV) atomicMin(&S.finv, i);
    }
  }
  if (ptid == SNT - 1) {  // the certificate of the piece open at the tile's end (fa_w_tcert)
    // (the first '\n' after the last '>': two mask words in one LDS round, the loop beyond)
    const u32 wi = alast >> 6;
    const u64 w0 = wi < (u32)(TILE / 64) ? S.mnl[wi] & (~0ull << (alast & 63)) : 0ull;
    const u64 w1 = wi + 1 < (u32)(TILE / 64) ? S.mnl[wi + 1] : 0ull;
    u32 q = w0 ? (wi << 6) + ctz64(w0) : (w1 ? ((wi + 1) << 6) + ctz64(w1) : fa_find_nl(S.mnl, alast, tlen));
    if (q > tlen) q = tlen;
    S.tcert = (q > alast && q + 1 < tlen && ascii_nonspace(r[q - 1]) && ascii_nonspace(r[q + 1])) ? 1u : 0u;
  }
  if (cb.nrel - rel * (u32)TILE <= (u32)TILE && ptid == SNT - 1) {  // the slab's last tile: the EOF piece
    // [last '>' + 1, n), fasta.go:111 + :123-125
    const KArgs k = kargs();
    u32 *tw = k->tile_words + (u64)t * FAW;
    u32 est = FA_OK;  // a slab with a halo: its last record is closed there (k_fa_fixup)
    const u32 lo = alast;
    if (k->end > k->n || !k->eof) {
    } else if (lo != 0 || fs) {
      if (tlen > lo + 1 && fa_find_nl(S.mnl, lo, tlen) < tlen) est = fa_check(r, S.mnl, lo, tlen, false);
    } else {
      est = fa_check(r, S.mnl, 0, tlen, true);
    }
    tw[6] = est;
    tw[7] = lo;
  }
  __builtin_amdgcn_s_setprio(0);
  lds_barrier();  // S.finv final; the slot and S are reused next
  {  // one packed word per tile (fa_word); the first invalid piece in tw[] (rare)
    const u32 finv = S.finv;
    const u64 word = fa_word(A, ncand, slow, delta, delta ? (S.cand[0] & 0x3FFFu) : FA_NONE,
                             (A >> 3) ? (S.cand[delta] & 0x3FFFu) : FA_NONE, finv != FA_NONE, S.tcert != 0);
    if (ptid == 0) p.tile_agg[t] = word;
    if (ptid == 0 && finv != FA_NONE) {
      u32 *tw = kargs()->tile_words + (u64)t * FAW;
      tw[4] = finv;
      tw[5] = S.cand[finv] >> 14;
    }
  }
}

// one LDS slot, claims of up to 32 consecutive tiles taken in file order (as k_fq_tiles): in one
// process over three copies of the C3 input (profiles/r06/calls/j/ab_fa_rr32.json) batches of 32
// dealt round-robin ran 1.858-1.994 ms against 1.896-2.020 for single tiles in XCD-major
// grid-stride order (round 5)
#ifndef SIDX_FA_WGS
// the compiler's bound; the grid follows the occupancy query (tile_grid): 19.1 KiB of LDS (no halo in the slot)
// and 63 VGPRs let 8 workgroups per CU in.  Held at 7 per CU the pass ran between 1.6 % faster and 6 % slower
// than at 8, the 8-per-CU contexts differing more among themselves (DESIGN.md §3 "Registers of the tile loop")
#define SIDX_FA_WGS 7
#endif
__global__ __launch_bounds__(SNT, SIDX_FA_WGS) void k_fa_tiles(const SlabParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[FRONT + TILE];
  __shared__ FaSmem S;
  if (gated_off(p)) return;  // format speculation failed: the host re-runs with the detected format
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  claim_loop(S.pad[0], tid, [&](u32 t, const ClaimRange &r, const ClaimBytes &cb) {
    fa_iter(p, cb, t - r.tb, S, raw, t, tid, lane, wid);
  });
}

// first boundary of tile u given its words and entering state: the conditional '>' when the
// tile is entered armed, else its first definite boundary (FA_NONE: none)
__device__ __forceinline__ u32 fa_first(u32 flags, u32 fc, u32 fd, u64 st) {
  return ((flags & 2) && (st & 1)) ? fc : fd;
}
// first boundary in tiles >= u (the whole wave, 64 tiles per step), n if none
__device__ u64 fa_next_global(const SlabParams &p, u64 u, int lane) {
  for (; u < p.ntiles; u += 64) {
    const u64 v = u + (u64)lane;
    u32 f = FA_NONE;
    if (v < p.ntiles) {
      const u64 w = p.tile_agg[v];
      f = fa_first(fa_w_flags(w), fa_w_fc(w), fa_w_fd(w), FastaMonoid::apply(p.state_in, p.tile_excl[v]));
    }
    const u64 bal = __ballot(f != FA_NONE);
    if (bal) {
      const int L = (int)ctz64(bal);
      return (u + (u64)L) * TILE + (u32)__shfl((int)f, L, 64);
    }
  }
  return p.n;
}

// k_fa_place: 64 consecutive tiles per workgroup, their words and entering states in LDS
// (plus the next tile's, for the row that crosses the group's end); a wave per tile.
__global__ __launch_bounds__(256) void k_fa_place(const SlabParams p) {
  __shared__ uint4 sw[PLACE_TILES + 1][2];
  __shared__ u64 sS[PLACE_TILES + 1];
  __shared__ u32 sC[PLACE_TILES];  // sC[k]: tile t0 + k - 1 certified the piece open at its end
  if (gated_off(p)) return;  // format speculation failed: the host re-runs with the detected format
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (u64 t0 = (u64)blockIdx.x * PLACE_TILES; t0 < p.ntiles; t0 += (u64)gridDim.x * PLACE_TILES) {
    if (tid >= 128 && tid < 128 + PLACE_TILES) {
      const u64 u = t0 + (u64)(tid - 128);  // the tile before t0 + (tid - 128), plus one
      sC[tid - 128] = (u >= 1 && u - 1 < p.ntiles) ? (u32)fa_w_tcert(p.tile_agg[u - 1]) : 0u;
    }
    if (tid <= PLACE_TILES && t0 + tid < p.ntiles) {
      const u64 w = p.tile_agg[t0 + tid];
      const u32 *tw = p.tile_words + (t0 + tid) * FAW;
      const bool last = t0 + tid == p.ntiles - 1;
      sw[tid][0] = make_uint4((u32)(w >> 18) & 0xFFFu, fa_w_flags(w), fa_w_fc(w), fa_w_fd(w));
      sw[tid][1] = make_uint4((w >> 63) ? tw[4] : FA_NONE, (w >> 63) ? tw[5] : 0u, last ? tw[6] : FA_OK,
                              last ? tw[7] : 0u);
      sS[tid] = FastaMonoid::apply(p.state_in, p.tile_excl[t0 + tid]);
    }
    __syncthreads();
    // four tiles per wave, 16 lanes each (a FASTA tile has ~10 boundaries): the tiles' stage
    // reads and row writes are in flight together instead of one tile's after another's
    const int sub = lane >> 4, sl = lane & 15;
    for (int kb = wid * 4; kb < PLACE_TILES; kb += 16) {
      const int k = kb + sub;  // <= PLACE_TILES - 1: sw[k + 1] is loaded
      const u64 t = t0 + k;
      const bool live = t < p.ntiles;
      if (!__ballot(live)) break;
      const uint4 w0 = sw[k][0], w1 = sw[k][1];
      const u32 ncand = w0.x, flags = w0.y, finv = w1.x, invlo = w1.y, est = w1.z, elo = w1.w;
      const u64 st = sS[k];
      const u64 cnt = st >> 1;
      const u64 tlo = t * TILE;
      if (p.n == 0) {  // no record at all: (0, EOF) on record 0
        if (lane == 0 && p.file_start) g_min64(p.badkey, bad_key(0, 0, ST_ABSENT));
        continue;
      }
      // too many candidates for the table: the whole tile from global memory
      if (live && (flags & 1) && sl == 0) push_fix(p, ~0ull, st, (u32)t);
      const bool go = live && !(flags & 1);
      const u32 skip = ((flags & 2) && !(st & 1)) ? 1u : 0u;
      const u32 nb = go ? ncand - skip : 0u;
      // end of the record open at the tile's end: the first boundary of a later tile
      u64 nxt = p.n;
      const bool wantn = go && (nb || t == 0) && t + 1 < p.ntiles;
      u32 f = FA_NONE;
      if (wantn) {
        const uint4 x = sw[k + 1][0];
        f = fa_first(x.y, x.z, x.w, sS[k + 1]);
        if (f != FA_NONE) nxt = (t + 1) * TILE + f;
      }
      // a later tile's first boundary: the whole wave searches, one group at a time
      u64 far = __ballot(wantn && f == FA_NONE && sl == 0);
      while (far) {
        const int L = (int)ctz64(far);
        far &= far - 1;
        const u64 tt = t0 + (u64)(kb + (L >> 4));
        const u64 r = fa_next_global(p, tt + 2, lane);
        if (sub == (L >> 4)) nxt = r;
      }
      const uint16_t *stage = reinterpret_cast<const uint16_t *>(p.tile_stage + t * RCAP);
      // the record open at a slab's start (number s0) is the previous slab's: no report of the
      // piece that closes it; if that was the tile's first invalid piece, the later invalid
      // ones of the tile go to k_fa_fixup (their piece starts are not kept)
      const u64 s0 = p.file_start ? ~0ull : (p.state_in >> 1);
      const bool finv_gone = finv != FA_NONE && finv >= skip && cnt + (finv - skip) == s0;
      for (u32 i = (u32)sl; i < nb; i += 16) {
        const u32 idx = i + skip;
        const u32 v = stage[idx];
        const u32 g = v & 0x3FFFu, vs = (v >> 14) & 3u;
        const u64 k2 = cnt + i;  // the record this '>' closes
        if (k2 == s0) {
        } else if (vs == FA_DEFER && idx == 0 && sC[k]) {
          // the tile's first '>' closes a piece that began before the tile: the previous tile
          // found a '\n' between two ASCII non-space bytes inside it (fa_w_tcert), so it is valid
        } else if (vs == FA_DEFER || (vs == FA_INV && finv_gone)) {
          push_fix(p, tlo + g, k2, (u32)t);
        } else if (vs == FA_INV && idx == finv) {  // the tile's first invalid piece
          p.detail[2 * t] = p.base + tlo + invlo;  // file offsets (slabs: base)
          p.detail[2 * t + 1] = g + 1 - invlo;  // the piece includes its '>'
          g_min64(p.badkey, bad_key(k2, (u32)t, ST_FA_INVALID));
        }
        const u64 e = (i + 1 < nb) ? tlo + (stage[idx + 1] & 0x3FFFu) : nxt;
        if (e == p.n && p.end > p.n) push_fix(p, tlo + g, k2 + 1, (u32)t | FIX_HALO);  // ends past the slab
        else put_row(p, k2 + 1, tlo + g, e - tlo - g);
      }
      if (go && t == 0 && sl == 0 && p.file_start) {  // record 0 starts at file offset 0
        const u64 e0 = nb ? (stage[skip] & 0x3FFFu) : nxt;
        if (e0 == p.n && p.end > p.n) push_fix(p, 0, 0, FIX_HALO);
        else put_row(p, 0, 0, e0);
      }
      if (go && p.eof && p.end == p.n && t == p.ntiles - 1 && sl == 0 && cnt + nb != s0) {  // closed by EOF
        const u64 k2 = cnt + nb;
        if (est == FA_INV) {
          const u32 slot = p.ntiles;
          p.detail[2 * (u64)slot] = p.base + tlo + elo;
          p.detail[2 * (u64)slot + 1] = p.n - tlo - elo;
          g_min64(p.badkey, bad_key(k2, slot, ST_FA_INVALID));
        } else if (est == FA_DEFER) {
          push_fix(p, p.n, k2, (u32)t);
        }
      }
    }
    __syncthreads();
  }
}

// position + 1 of the last '>' in [0, pos), 0 if none (the whole wave, 1 KiB per step)
__device__ u64 fa_prev_gt(const SlabParams &p, u64 pos, int lane) {
  if (pos == 0) return 0;
  u64 top = (pos - 1) & ~15ull;  // the chunk holding byte pos - 1
  const u64 off = 16ull * (u64)(63 - lane);
  for (;;) {
    u32 m = 0;
    u64 a = 0;
    if (top >= off) {
      a = top - off;
      const uint4 v = (a + 16 <= p.end) ? load16(p.data + a) : load16_partial(p.data, a, p.end);
      m = eq16(v, '>');
      if (a + 16 > pos) m &= (1u << (u32)(pos - a)) - 1u;
    }
    const u64 bal = __ballot(m != 0);
    if (bal) {
      const int L = 63 - (int)clz64(bal);
      const u64 q = m ? a + 31 - (u64)__builtin_clz(m) : 0ull;
      return __shfl(q, L, 64) + 1;
    }
    if (top < 1024) return 0;
    top -= 1024;
  }
}

__device__ __forceinline__ void fa_report(const SlabParams &p, u64 k, u32 slot, u64 epos, u64 elen, int lane) {
  if (lane == 0) {
    p.detail[2 * (u64)slot] = p.base + epos;  // file offset
    p.detail[2 * (u64)slot + 1] = elen;
    g_min64(p.badkey, bad_key(k, slot, ST_FA_INVALID));
  }
}

// FASTA slab with a halo (end > n): the record opened at b (number k) ends at the first
// boundary at or after n -- a '>' with a '\n' since the '>' before it -- found in the halo
// [n, end) from the slab's final armed bit, 1 KiB per step (per lane: the first boundary of its
// 16 bytes given the armed bit it is entered with, which is the last '\n' / '>' event of the
// lanes before it).  Its closing piece is validated and its row written here; a halo without a
// boundary that does not reach EOF is ST_NEEDMORE (the slab protocol's "halo exhausted").
__device__ void fa_halo_close(const SlabParams &p, u64 b, u64 k, u32 slot, int lane) {
  const u64 nt = p.ntiles;
  u32 armed = (u32)(FastaMonoid::apply(FastaMonoid::apply(p.state_in, p.tile_excl[nt - 1]), p.tile_agg[nt - 1] & FAW_AMASK) & 1);
  WaveAcc wa;
  wa.g = p.data; wa.end = p.end; wa.eof = p.eof; wa.lane = lane; wa.front = p.front;
  u64 g = ~0ull;
  for (u64 c0 = p.n & ~15ull; c0 < p.end && g == ~0ull; c0 += 1024) {
    const u64 a = c0 + 16ull * (u64)lane;
    u32 nl = 0, gt = 0;
    if (a < p.end) {
      const uint4 v = (a + 16 <= p.end) ? load16(p.data + a) : load16_partial(p.data, a, p.end);
      const u32 keep = a < p.n ? ~((1u << (u32)(p.n - a)) - 1u) & 0xFFFFu : 0xFFFFu;  // bytes >= n only
      nl = eq16(v, '\n') & keep;
      gt = eq16(v, '>') & keep;
    }
    // the lane's effect on the armed bit: 0 none, 1 clears ('>' last), 2 sets ('\n' last)
    const u32 hi_nl = nl ? 32 - __builtin_clz(nl) : 0u, hi_gt = gt ? 32 - __builtin_clz(gt) : 0u;
    const u32 eff = (nl | gt) ? (hi_nl > hi_gt ? 2u : 1u) : 0u;
    // armed bit entering the lane: the effect of the nearest lane below with one, else `armed`
    const u32 key = eff ? ((u32)lane + 1) * 4 + eff : 0u;
    u32 mx = key;
    for (int d = 1; d < 64; d <<= 1) {
      const u32 y = (u32)__shfl_up((int)mx, d, 64);
      if (lane >= d && y > mx) mx = y;
    }
    u32 below = (u32)__shfl_up((int)mx, 1, 64);
    if (lane == 0) below = 0;
    u32 in = below ? ((below & 3u) == 2u) : armed;
    u32 hit = 16;
    for (u32 m = gt; m; m &= m - 1) {
      const u32 j = (u32)__builtin_ctz(m);
      const u32 prevgt = gt & ((1u << j) - 1u);
      const u32 since = prevgt ? (nl & ~((2u << (31 - __builtin_clz(prevgt))) - 1u)) : nl;
      if ((since & ((1u << j) - 1u)) || (!prevgt && in)) { hit = j; break; }
    }
    const u64 hb = __ballot(hit < 16);
    if (hb) {
      const int L = (int)ctz64(hb);
      g = c0 + 16ull * (u64)L + (u32)__shfl((int)hit, L, 64);
    } else {
      const u32 last = (u32)__shfl((int)mx, 63, 64);
      if (last) armed = (last & 3u) == 2u;
    }
  }
  if (g == ~0ull && !p.eof) {
    if (lane == 0) g_min64(p.badkey, bad_key(k, slot, ST_NEEDMORE));
    return;
  }
  const u64 e = g == ~0ull ? p.end : g;
  const u64 lo = fa_prev_gt(p, e, lane);
  bool ok = true;
  u64 q;
  if (g != ~0ull) fasta_piece_ok(wa, lo, g, ok);
  else if (p.end - lo > 1 && wa.find(C_NL, lo, p.end, q) == FR_FOUND) fasta_piece_ok(wa, lo, p.end, ok);
  if (lane == 0) put_row(p, k, b, e - b);
  if (!ok) fa_report(p, k, slot, lo, g == ~0ull ? p.end - lo : g + 1 - lo, lane);
}

// k_fa_fixup: one wave per queued item.  A piece closing record k at b (b == n: the EOF
// piece) re-checked with the general validator; or a whole tile (start == ~0, g = its
// entering state) walked '>' by '>' from global memory.  Each item reports into a detail
// slot of its own (tiles: the tile; pieces: fixcap + item), so the first-bad record's text
// is never overwritten by another report.
__global__ __launch_bounds__(256) void k_fa_fixup(const SlabParams p, DevResult *res) {
  if (gated_off(p)) {
    if (res) last_block_finalize(p, F_FASTA, res);
    return;
  }
  const int lane = threadIdx.x & 63;
  const u32 nw = gridDim.x * (blockDim.x / 64);
  const u32 wv = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const u32 nq = p.counters[2] < p.fixcap ? p.counters[2] : (u32)p.fixcap;
  WaveAcc wa;
  wa.g = p.data; wa.end = p.end; wa.eof = p.eof; wa.lane = lane; wa.front = p.front;
  const u64 s0 = p.file_start ? ~0ull : (p.state_in >> 1);  // the previous slab's record (see k_fa_place)
  for (u32 i = wv; i < nq; i += nw) {
    const FixRec f = reinterpret_cast<const FixRec *>(p.fix)[i];
    if (f.tile & FIX_HALO) {
      fa_halo_close(p, f.start, f.g, p.fixcap + i, lane);
      continue;
    }
    if (f.start != ~0ull) {
      if (f.g == s0) continue;
      const u64 b = f.start;
      const u64 lo = fa_prev_gt(p, b, lane);
      bool ok = true;
      u64 elen = 0;
      if (b == p.n) {  // EOF piece: validated iff longer than 1 byte and holding a '\n'
        u64 q;
        if (p.n - lo > 1 && wa.find(C_NL, lo, p.n, q) == FR_FOUND) fasta_piece_ok(wa, lo, p.n, ok);
        elen = p.n - lo;
      } else {
        fasta_piece_ok(wa, lo, b, ok);
        elen = b + 1 - lo;
      }
      if (!ok) fa_report(p, f.g, p.fixcap + i, lo, elen, lane);
      continue;
    }
    const u64 t = f.tile;
    u64 cnt = f.g >> 1;
    bool armed = f.g & 1;
    const u64 tlo = t * TILE, thi = (tlo + TILE < p.n) ? tlo + TILE : p.n;
    u64 lo = fa_prev_gt(p, tlo, lane);
    u64 pend = (t == 0 && p.file_start) ? 0 : ~0ull, pk = 0;  // the open row (start, record number)
    u64 pos = tlo;
    bool bad = false;
    for (;;) {
      u64 g, q;
      if (wa.find(C_X, pos, thi, g) != FR_FOUND) break;
      if (!armed) armed = wa.find(C_NL, pos, g, q) == FR_FOUND;
      if (armed) {
        bool ok = true;
        if (cnt != s0) fasta_piece_ok(wa, lo, g, ok);
        if (!ok) {
          fa_report(p, cnt, (u32)t, lo, g + 1 - lo, lane);
          bad = true;
          break;
        }
        if (pend != ~0ull && lane == 0) put_row(p, pk, pend, g - pend);
        ++cnt;
        pend = g;
        pk = cnt;
        armed = false;
      }
      lo = g + 1;
      pos = g + 1;
    }
    if (bad) continue;  // later records are past the first bad one
    if (pend != ~0ull) {
      const u64 e = fa_next_global(p, t + 1, lane);
      if (e == p.n && p.end > p.n) fa_halo_close(p, pend, pk, p.fixcap + i, lane);
      else if (lane == 0) put_row(p, pk, pend, e - pend);
    }
    if (t == p.ntiles - 1 && p.eof && p.end == p.n && cnt != s0) {
      bool ok = true;
      u64 q;
      if (p.n - lo > 1 && wa.find(C_NL, lo, p.n, q) == FR_FOUND) fasta_piece_ok(wa, lo, p.n, ok);
      if (!ok) fa_report(p, cnt, (u32)t, lo, p.n - lo, lane);
    }
  }
  if (res) last_block_finalize(p, F_FASTA, res);
}

// ====================================================================================
// k_finalize: slab result; resets the other build's first-bad slot and counters
// ====================================================================================
template <class M>
__device__ __forceinline__ u64 apply_fmt(u64 s, u64 a) { return M::apply(s, a); }

__device__ __forceinline__ void finalize_body(const SlabParams &p, int fmt, DevResult *res);
__global__ void k_finalize(const SlabParams p, int fmt, DevResult *res) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  finalize_body(p, fmt, res);
}
// k_finalize's body (thread 0 of one workgroup): also run by the last workgroup of k_fixup
__device__ __forceinline__ void finalize_body(const SlabParams &p, int fmt, DevResult *res) {
  if (gated_off(p)) {  // the speculated format was wrong: nothing ran; the host re-runs
    DevResult r = {};
    r.flags = RF_MISSPEC;
    r.fmt = (u32)fmt;
    r.detected = (u32)*p.gate;
    *res = r;
    *p.badkey_next = KEY_NONE;
    for (int i = 0; i < NCOUNTERS; ++i) p.counters_next[i] = 0;
    return;
  }
  const u64 w = ((volatile u64 *)p.status)[p.ntiles - 1];
  const u64 agg = w & PAYLOAD_MASK;  // slab aggregate
  u64 fin;
  // (k_fixup's last workgroup: the other workgroups' first-bad keys are device-scope atomics)
  if (fmt == F_FASTA) fin = apply_fmt<FastaMonoid>(p.state_in, agg);
  else if (fmt == F_SAM) fin = apply_fmt<SamMonoid>(p.state_in, agg);
  else fin = apply_fmt<CountMonoid>(p.state_in, agg);
  const u64 key = __hip_atomic_load(p.badkey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  DevResult r;
  r.state_out = fin;
  r.slab_agg = agg;
  r.err_pos = 0;
  r.err_len = 0;
  r.flags = 0;
  r.path = 0;
  r.fixups = p.counters[2];
  r.fix_tiles = p.counters[3] >> 1;
  r.fmt = (u32)fmt;
  r.detected = p.gate ? (u32)*p.gate : 0u;
  r.pad = 0;
  r.key = key;
  if ((w >> 62) != 2 || (((u32)(w >> EPOCH_SHIFT)) & EPOCH_MASK) != p.epoch) r.flags |= RF_INTERNAL;  // no final INC
  u64 krec = key >> KEY_REC_SHIFT;
  u32 kst = (u32)(key & 15);
  const u32 ktile = (u32)((key >> 4) & ((1u << KEY_TILE_BITS) - 1));
  const u64 natural = natural_count(fmt, fin);  // count when no record terminates the sequence early
  r.natural = natural;
  if (key == KEY_NONE) {
    r.count = natural;
    r.code = ST_OK;
  } else {
    r.count = krec;
    r.code = kst;
    if (kst == ST_FA_INVALID) {
      r.err_pos = p.detail[2 * (u64)ktile];
      r.err_len = p.detail[2 * (u64)ktile + 1];
    }
    if (kst == ST_DONTCARE) r.flags |= RF_INTERNAL;
    if (kst == ST_NEEDMORE) r.flags |= RF_HALO;
  }
  if (p.counters[1]) r.flags |= RF_INTERNAL;
  if (p.counters[3] & 1) r.flags |= RF_FIXQUEUE;  // k_fixup queue overflow: re-run on the general kernel
  if (p.inject & 1) r.count = r.count ? r.count - 1 : 0;  // test hook: a short count
  const u64 nrows = r.count > p.row_base ? r.count - p.row_base : 0;
  if (nrows > p.row_cap) r.flags |= RF_CAPACITY;
  // End-of-build invariants of a whole-file build (record.go:51-83: row i + 1 starts where row i
  // ends, the first at 0).  A successful FASTA / SAM / line build consumes every byte, so its last
  // row ends at the file end; a FASTQ build only skips trailing blank lines after its last record
  // (fastq.go:141-156).  A build whose count or rows came out of stale device state fails here
  // and reports an internal error instead of a short table.
  if (p.file_start && p.eof && p.end == p.n && !(r.flags & (RF_CAPACITY | RF_FIXQUEUE)) && nrows && p.rows) {  // (p.end > p.n: a slab's halo)
    const u64 *rw = p.rows;
    bool bad = rw[0] != p.base;
    if (r.code == ST_OK || r.code == ST_END || r.code == ST_ABSENT) {
      const u64 e = rw[2 * (nrows - 1)] + rw[2 * (nrows - 1) + 1], fe = p.base + p.n;
      if (fmt == F_FASTQ) bad |= e > fe || (e < fe && (p.data[e - p.base] != '\n' || p.data[p.n - 1] != '\n'));
      else bad |= e != fe;
      // the line index's last row is the bytes after the last '\n' (line.go:37-45, possibly none)
      if (fmt == F_LINE) bad |= rw[2 * (nrows - 1) + 1] != 0 && p.n && p.data[p.n - 1] == '\n';
    }
    if (bad) r.flags |= RF_INTERNAL;
  }
  *res = r;
  if (p.summary) {
    SlabSummary *o = reinterpret_cast<SlabSummary *>(p.summary);
    o->agg = agg; o->state_in = p.state_in; o->key = key; o->natural = natural;
    o->row_base = p.row_base; o->err_pos = r.err_pos; o->err_len = r.err_len;
    o->fmt = (uint16_t)fmt; o->flags = (uint16_t)r.flags; o->seq = p.seq;
  }
  *p.badkey_next = KEY_NONE;
  for (int i = 0; i < NCOUNTERS; ++i) p.counters_next[i] = 0;
}

// ====================================================================================
// k_scan_excl<M>: the device-wide exclusive scan of the per-tile monoid aggregates -- the
// parallel form of record.go:76's serial `curr += int64(n)` (the global record number of a
// tile's first record is the fold of everything before it).  Single pass, decoupled
// look-back: 2048 aggregates per workgroup (8 per thread, thread -> wave -> block scans),
// the block's aggregate published as an epoch-tagged status word, then wave 0 folds its
// predecessors' words 64 at a time back to the nearest inclusive one.  Workgroups take their
// block number from a per-build ticket, so a block only ever waits on blocks that were
// already running (no residency assumption).  The block holding the last tile also writes
// the slab aggregate where k_finalize reads it (status[ntiles - 1]).
// ====================================================================================
constexpr int SCAN_T = 256, SCAN_ITEMS = 8, SCAN_BLOCK = SCAN_T * SCAN_ITEMS;

template <class M>
__global__ __launch_bounds__(SCAN_T) void k_scan_excl(const u64 *agg, u64 *excl, u32 n, u64 *look, u32 *ticket,
                                                      u64 *total_word, u32 epoch, u64 in_mask, const int *gate,
                                                      int gate_fmt) {
  __shared__ u64 wtot[SCAN_T / 64];
  __shared__ u64 bpre;
  __shared__ u32 sbid;
  if (gate && *gate != gate_fmt) return;  // format speculation failed (no ticket taken)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) sbid = __hip_atomic_fetch_add((gu32 *)ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const u32 bid = sbid;
  const u64 i0 = (u64)bid * SCAN_BLOCK + (u64)tid * SCAN_ITEMS;
  u64 v[SCAN_ITEMS];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) v[k] = (i0 + k < n) ? (agg[i0 + k] & in_mask) : M::identity();
#pragma unroll
  for (int k = 1; k < SCAN_ITEMS; ++k) v[k] = M::combine(v[k - 1], v[k]);
  const u64 tinc = wave_incl_scan<M>(v[SCAN_ITEMS - 1], lane);
  u64 texc = __shfl_up(tinc, 1, 64);
  if (lane == 0) texc = M::identity();
  if (lane == 63) wtot[wid] = tinc;
  __syncthreads();
  u64 wpre = M::identity(), btot = M::identity();
#pragma unroll
  for (int w = 0; w < SCAN_T / 64; ++w) {
    if (w < wid) wpre = M::combine(wpre, wtot[w]);
    btot = M::combine(btot, wtot[w]);
  }
  if (wid == 0) {
    gu64 *lk = (gu64 *)look;
    const u64 tag = (u64)epoch << EPOCH_SHIFT;
    u64 pre = M::identity();
    if (bid == 0) {
      if (lane == 0) st_store(lk, FLAG_INC | tag | btot);
    } else {
      if (lane == 0) st_store(lk + bid, FLAG_AGG | tag | btot);
      u64 acc = M::identity();  // fold of the blocks between the window and this one
      i64 hi = (i64)bid - 1;    // newest block of the window (lane 0)
      for (;;) {
        const i64 idx = hi - lane;
        u64 w = idx >= 0 ? st_load(lk + idx) : (FLAG_INC | tag | M::identity());
        u64 incm, zm;
        for (;;) {
          const u32 f = wflag(w, epoch);
          incm = __ballot(f == 2);
          zm = __ballot(f == 0);
          const u64 need = incm ? lowmask(ctz64(incm)) : ~0ull;  // lanes newer than the INC
          if (!(zm & need)) break;
          __builtin_amdgcn_s_sleep(1);
          if (f == 0) w = st_load(lk + idx);
        }
        const u32 fi = incm ? ctz64(incm) : 64u;
        const u64 x = ((u32)lane <= fi) ? (w & PAYLOAD_MASK) : M::identity();
        const u64 fold = __shfl(wave_fold_newest_first<M>(x, lane), 0, 64);
        acc = M::combine(fold, acc);
        if (incm) break;
        hi -= 64;
      }
      pre = acc;
      if (lane == 0) st_store(lk + bid, FLAG_INC | tag | M::combine(pre, btot));
    }
    if (lane == 0) {
      bpre = pre;
      if ((u64)bid * SCAN_BLOCK < n && (u64)(bid + 1) * SCAN_BLOCK >= n)  // the block of the last tile
        st_store((gu64 *)total_word, FLAG_INC | tag | M::combine(pre, btot));
    }
  }
  __syncthreads();
  const u64 base = M::combine(bpre, M::combine(wpre, texc));
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k)
    if (i0 + k < n) excl[i0 + k] = k ? M::combine(base, v[k - 1]) : base;
}

}  // namespace sidx

// ====================================================================================
// Host launch wrappers (internal to libshockidx, declared in sidx_launch.hpp; the build path is
// chosen in sidx_build.cpp, the control kernels' launchers are in sidx_control.hip)
// ====================================================================================
using namespace sidx;

namespace {
// The persistent grid of a tile kernel: CUs x its own co-resident workgroups (the launch
// parameters' pgrid is sized for k_fq_tiles; a larger grid than fits would leave the extra
// workgroups to start after the others finish their whole tile sequence).
template <class K>
int occupancy(K kern) {
  int n = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, SNT, 0) == hipSuccess && n > 0 ? n : 1;
}
u32 tile_grid(const SlabParams &p, TilePass pass) {
  // cached per device and kernel; written from the multi-device slab threads at once, so the
  // cache words are atomics (a repeated query stores the same value)
  static std::atomic<int> occ[TP_SAM + 1], cus[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::atomic<int> &cu_slot = cus[dev & 63];
  int cu = cu_slot.load(std::memory_order_relaxed);
  if (!cu) {
    (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
    cu_slot.store(cu, std::memory_order_relaxed);
  }
  int oc = occ[pass].load(std::memory_order_relaxed);
  if (!oc) {
    oc = pass == TP_FA ? occupancy(k_fa_tiles) : pass == TP_SAM ? occupancy(k_sam_tiles) : occupancy(k_line_tiles);
    occ[pass].store(oc, std::memory_order_relaxed);
  }
  const u64 g = (u64)(cu > 0 ? cu : 1) * (u64)(oc > 0 ? oc : 1);
  return (u32)(g < p.ntiles ? g : p.ntiles);
}
// grid of a placement kernel that takes `per` tiles per workgroup and strides by its grid
u32 place_grid(u64 ntiles, u64 per) {
  const u64 g = (ntiles + per - 1) / per;
  return (u32)(g < 65536 ? g : 65536);
}
// look-back words of the scans: two arrays of the status block (SlabParams::scan_look)
template <class M>
hipError_t scan_excl(const SlabParams &p, const u64 *agg, u64 *excl, int which, bool total, hipStream_t s,
                     u64 in_mask = ~0ull) {
  const u32 nb = (p.ntiles + SCAN_BLOCK - 1) / SCAN_BLOCK;
  hipLaunchKernelGGL(k_scan_excl<M>, dim3(nb ? nb : 1), dim3(SCAN_T), 0, s, agg, excl, p.ntiles,
                     p.scan_look[which], p.counters + 4 + which, total ? p.status + (p.ntiles - 1) : p.scan_look[which] + nb,
                     p.epoch, in_mask, p.gate, p.gate_fmt);
  return hipGetLastError();
}
hipError_t finalize(const SlabParams &p, int fmt, DevResult *d_res, hipStream_t s) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, s, p, fmt, d_res);
  return hipGetLastError();
}

// Two-pass index (SAM slabs; the general re-run; *_MODE=two): pass 1 (tile aggregates, their
// exclusive scan, the slab aggregate) then k_index1 with every tile's incoming state.
template <int F>
hipError_t launch_two_pass(const SlabParams &p, DevResult *d_res, hipStream_t s, hipEvent_t ek0, hipEvent_t ek1) {
  const dim3 g1(p.ntiles), block(NTHREADS);
  if (ek0) (void)hipEventRecord(ek0, s);
  hipLaunchKernelGGL(k_tile_agg<F>, g1, block, 0, s, p, p.tile_agg);
  hipError_t e = scan_excl<typename Traits<F>::M>(p, p.tile_agg, (u64 *)p.tile_excl, 0, true, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_index1<F>, g1, block, 0, s, p);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (ek1) (void)hipEventRecord(ek1, s);
  return finalize(p, F, d_res, s);
}

constexpr u32 FIX_GRID = 64;  // k_fixup workgroups: the queue is short on real data (a few items per 10 GiB)
// The FASTQ tile pass: k_fq_tiles, the exclusive scan of the tile newline counts (and the
// slab aggregate), k_fq_place, k_fixup (which finalizes the build).  index_ms (ek0 -> ek1)
// covers k_fq_tiles alone, on the grid the caller sized for it (sidx_tiles_blocks_per_cu).
hipError_t launch_fq(const SlabParams &p, DevResult *d_res, hipStream_t s, hipEvent_t ek0, hipEvent_t ek1) {
  // ek0 / ek1 time the tile pass alone: recorded by its dispatch packet (hipExtLaunchKernel),
  // not as separate stream packets that would add their own gaps to the build
  if (p.fq_lines) hipExtLaunchKernelGGL(k_fq_tiles<true>, dim3(p.pgrid), dim3(SNT), 0, s, ek0, ek1, 0, p);
  else hipExtLaunchKernelGGL(k_fq_tiles<false>, dim3(p.pgrid), dim3(SNT), 0, s, ek0, ek1, 0, p);
  hipError_t e = scan_excl<CountMonoid>(p, p.tile_agg, (u64 *)p.tile_excl, 0, true, s, FQW_TMASK);
  if (e != hipSuccess) return e;
  // test hook (SHOCKIDX_DEBUG bit 12): fail after the scan, as a launch error there would --
  // the build's ticket / first-bad slot is then left unreset (tests/test_gpu_host.py)
  if (p.debug & 4096u) return hipErrorLaunchFailure;
  hipLaunchKernelGGL(k_fq_place, dim3(place_grid(p.ntiles, PLACE_TILES)), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_fixup, dim3(FIX_GRID), dim3(256), 0, s, p, d_res);
  return hipGetLastError();
}

// The FASTA tile pass: k_fa_tiles, the FastaMonoid scan of the tile aggregates, k_fa_place,
// k_fa_fixup (which finalizes the build).
hipError_t launch_fa(const SlabParams &p, DevResult *d_res, hipStream_t s, hipEvent_t ek0, hipEvent_t ek1) {
  hipExtLaunchKernelGGL(k_fa_tiles, dim3(p.pgrid), dim3(SNT), 0, s, ek0, ek1, 0, p);
  hipError_t e = scan_excl<FastaMonoid>(p, p.tile_agg, (u64 *)p.tile_excl, 0, true, s, FAW_AMASK);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_fa_place, dim3(place_grid(p.ntiles, PLACE_TILES)), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_fa_fixup, dim3(FIX_GRID), dim3(256), 0, s, p, d_res);
  return hipGetLastError();
}

// The line tile pass: k_line_tiles, the count scan (row bases, slab aggregate) and the max
// scan of the last '\n' + 1 (each tile's first row start), k_line_place, k_line_final.
hipError_t launch_line(const SlabParams &p, DevResult *d_res, hipStream_t s, hipEvent_t ek0, hipEvent_t ek1) {
  hipExtLaunchKernelGGL(k_line_tiles, dim3(p.pgrid), dim3(SNT), 0, s, ek0, ek1, 0, p);
  hipError_t e = scan_excl<CountMonoid>(p, p.tile_agg, (u64 *)p.tile_excl, 0, true, s, LCOUNT);
  if (e == hipSuccess) e = scan_excl<MaxMonoid>(p, p.pcnt, p.ppre, 1, false, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_line_place<F_LINE>, dim3(place_grid(p.ntiles, LPLACE_TILES)), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_line_final, dim3(1), dim3(64), 0, s, p);
  return finalize(p, F_LINE, d_res, s);
}

// The SAM tile pass (single-slab builds): k_sam_tiles, the SamMonoid scan (incoming states,
// the slab aggregate), k_sam_resolve, the max scan of the last terminator + 1, placement,
// k_sam_final.
hipError_t launch_sam(const SlabParams &p, DevResult *d_res, hipStream_t s, hipEvent_t ek0, hipEvent_t ek1) {
  hipExtLaunchKernelGGL(k_sam_tiles, dim3(p.pgrid), dim3(SNT), 0, s, ek0, ek1, 0, p);
  hipError_t e = scan_excl<SamMonoid>(p, p.tile_agg, (u64 *)p.tile_excl, 0, true, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sam_resolve, dim3((p.ntiles + 255) / 256), dim3(256), 0, s, p);
  e = scan_excl<MaxMonoid>(p, p.pcnt, p.ppre, 1, false, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_line_place<F_SAM>, dim3(place_grid(p.ntiles, LPLACE_TILES)), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_sam_final, dim3(1), dim3(64), 0, s, p);
  return finalize(p, F_SAM, d_res, s);
}
}  // namespace

// One slab's build on the path the host chose (sidx_build.cpp choose_pass); the two-pass build
// takes its format from the parameters (gate_fmt).  The FASTA, line and SAM tile kernels run on
// their own persistent grid (tile_grid), FASTQ on the caller's.
extern "C" hipError_t sidx_launch_tiles(TilePass pass, const SlabParams *pp, DevResult *d_res, hipStream_t s,
                                        hipEvent_t ek0, hipEvent_t ek1) {
  SlabParams p = *pp;
  if (pass == TP_FA || pass == TP_LINE || pass == TP_SAM) p.pgrid = tile_grid(p, pass);
  if (p.grid_cap && p.pgrid > p.grid_cap) p.pgrid = p.grid_cap;
  switch (pass) {
    case TP_FQ: return launch_fq(p, d_res, s, ek0, ek1);
    case TP_FA: return launch_fa(p, d_res, s, ek0, ek1);
    case TP_LINE: return launch_line(p, d_res, s, ek0, ek1);
    case TP_SAM: return launch_sam(p, d_res, s, ek0, ek1);
    case TP_TWO_PASS:
      switch (p.gate_fmt) {
        case F_FASTQ: return launch_two_pass<F_FASTQ>(p, d_res, s, ek0, ek1);
        case F_FASTA: return launch_two_pass<F_FASTA>(p, d_res, s, ek0, ek1);
        case F_SAM: return launch_two_pass<F_SAM>(p, d_res, s, ek0, ek1);
        case F_LINE: return launch_two_pass<F_LINE>(p, d_res, s, ek0, ek1);
      }
  }
  return hipErrorInvalidValue;
}

// u32 words of SlabParams::tile_stage a tile pass needs.  Line / SAM: LCAP u16 '\n' positions per
// tile.  FASTQ / FASTA: a slot of RCAP u32 per tile (FASTQ keeps FQ_LINE_E + FQ_OVF u16 starts in
// it, FASTA RCAP u16 candidates), with the persistent grid + 16 tiles of slack that an earlier
// layout needed (kept: the size feeds the device budget).
static_assert(FQ_LINE_E + FQ_OVF <= 2 * RCAP, "a FASTQ tile's starts fit its slot");
extern "C" u64 sidx_tile_stage_words(TilePass pass, u64 ntiles, u32 grid) {
  return (pass == TP_LINE || pass == TP_SAM) ? ntiles * (LCAP / 2) : (ntiles + grid + 16) * (u64)RCAP;
}

extern "C" hipError_t sidx_launch_fq_spans_place(const SlabParams *pp, u32 *spans, u64 *outlen, u64 K, int kind,
                                                hipStream_t s) {
  const SlabParams &p = *pp;
  if (!p.fq_lines || !p.ntiles) return hipSuccess;
  hipLaunchKernelGGL(k_fq_spans_place, dim3(place_grid(p.ntiles, 4)), dim3(256), 0, s, p, spans, outlen, K, kind);
  return hipGetLastError();
}

// Co-resident workgroups per CU of the FASTQ tile pass (its persistent grid = CUs x this).
extern "C" int sidx_tiles_blocks_per_cu() {
  int n = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_fq_tiles<false>, SNT, 0) == hipSuccess ? n : 0;
}
