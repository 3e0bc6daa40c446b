// sidx_column.hip -- the column index (index/column.go:33-130): a tab-separated file grouped by
// the runs of one column.  The general build, over the line index of the same bytes:
//
//   k_col_flags   per line: non-blank (longer than one byte, column.go:64)
//   (sum scan)    the non-blank lines' ranks
//   k_col_keys    per non-blank line: its key span (col_key), compacted by rank; the first line
//                 without the column is a 64-bit minimum over line offsets
//   k_col_cmp     per non-blank line: key != the previous non-blank line's key (column.go:80);
//                 lengths first, then 16 bytes at a time; a key above COL_WAVE_KEY bytes is
//                 compared by its whole wave
//   (sum scan)    the cuts' ranks
//   k_col_cuts    the cut offsets by rank
//   k_col_rows    rows (p_k, p_k+1 - p_k) from adjacent cuts, 0 and n at the ends
//   k_col_check   SHOCKIDX_VERIFY: the last row ends at n (k_verify_rows checks the rest)
//
// Every kernel runs over the line count L (an upper bound of the non-blank lines, the cuts and
// the rows) and reads the exact counts from the control words, so the host waits once.
//
// The tile pass reads the input once, in the shape of k_line_tiles (sidx_kernels.hip), through the
// same LDS-DMA staging (sidx_stage.hpp):
//
//   k_col_tiles   per 16 KiB tile, from LDS: '\n' and '\t' masks; every line that follows a '\n'
//                 of the tile (line 0: tile 0) is blank, or has its key found and compared with
//                 the previous non-blank line of the tile; the decided cuts (u16 line starts),
//                 and one word per tile: their count and the two lines it could not decide -- its
//                 first non-blank line (the predecessor is in an earlier tile) and the line that
//                 runs past its end -- plus the start of its last non-blank line
//   (max scan)    each tile's predecessor line: the last non-blank line before it, however many
//                 blank tiles lie between
//   k_col_fix     the two undecided lines per tile, with the general build's routines from
//                 global memory; the tile's cut total
//   (sum scan)    each tile's first cut number
//   k_col_place   cut k's offset into row k + 1
//   k_col_lens    row 0's offset and every length
//
// The slab pass is the tile pass over one slab of the file (n owned bytes, a halo readable past
// them), with what column.go's loop carries from line to line (column.go:44-48: curr, the rows so
// far, line_count != 0, prev_str) in a carry on the device:
//
//   k_col_tiles        as above, without line 0 unless the slab starts the file and without a
//                      "last piece" unless its owned bytes end it
//   k_col_fix<true>    bounded by the slab's readable end; a tile's first line without a
//                      predecessor in the slab is compared with the carried key (column.go:80);
//                      a line whose key does not close in the window is reported, not guessed
//   k_col_slab_sum     the cut total, the last non-blank owned line and its key, the rows
//   (host stop)        first bad line, first unsettled line, rows against the capacity
//   k_col_slab_place   cut k ends row k and starts row k + 1, at file offsets
//   k_col_slab_close   row k = (its start: row 0's is the carried cut, its length); the file's last
//                      slab closes the last row at the file's size (column.go:119-125)
//   k_col_slab_carry   the next carry into the half this slab did not read, then the flip
#include <hip/hip_runtime.h>
#include <string.h>

#include "sidx_common.hpp"
#include "sidx_device.hpp"
#include "sidx_launch.hpp"
#include "sidx_scan.hpp"
#include "sidx_stage.hpp"

namespace sidx {

constexpr u64 COL_WAVE_KEY = 4096;  // keys longer than this are compared by the whole wave
constexpr int COL_T = 256;

// 16 bytes at the 16-byte aligned a < n, zero-filled past n
__device__ __forceinline__ uint4 col_load16(const uint8_t *d, u64 a, u64 n) {
  return a + 16 <= n ? load16(d + a) : load16_partial(d, a, n);
}
// 16 bytes at any address (all inside the file)
__device__ __forceinline__ uint4 col_load16u(const uint8_t *p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// The key of the non-blank line [off, off + len) for column c >= 1 (column.go:74-79): the bytes
// after its (c-1)-th '\t' up to its c-th, or to the line's end (its '\n' included) when there is
// no c-th.  False: the line has fewer than c fields (klen = 0).  Reads global memory 16 aligned
// bytes at a time; a chunk whose tabs all lie before the key's first is only counted.
__device__ bool col_key(const uint8_t *d, u64 n, u64 off, u64 len, u32 c, u64 &lo, u64 &klen) {
  const u64 end = off + len;
  u64 t = 0;  // tabs seen
  lo = off;
  for (u64 a = off & ~15ull; a < end; a += 16) {
    u32 m = eq16(col_load16(d, a, n), '\t');
    if (a < off) m &= ~0u << (u32)(off - a);
    if (a + 16 > end) m &= (1u << (u32)(end - a)) - 1u;
    const u32 pc = (u32)__popc(m);
    if (t + pc + 1 < c) {
      t += pc;
      continue;
    }
    while (m) {
      const u64 pos = a + (u32)__builtin_ctz(m);
      m &= m - 1;
      if (++t == c) {
        klen = pos - lo;
        return true;
      }
      if (t + 1 == c) lo = pos + 1;
    }
  }
  if (t + 1 < c) {
    klen = 0;
    return false;
  }
  klen = end - lo;
  return true;
}

// bytes [a, a + len) differ from [b, b + len): the 16-byte pieces first, first + stride, ...
// (one lane: 0 and 16; a wave: 16 * lane and 1024)
__device__ bool col_differ2(const uint8_t *pa, const uint8_t *pb, u64 len, u64 first, u64 stride) {
  for (u64 m = first; m < len; m += stride) {
    if (len - m >= 16) {
      const uint4 x = col_load16u(pa + m), y = col_load16u(pb + m);
      if ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) return true;
    } else {
      for (u64 i = m; i < len; ++i)
        if (pa[i] != pb[i]) return true;
    }
  }
  return false;
}
__device__ __forceinline__ bool col_differ(const uint8_t *d, u64 a, u64 b, u64 len, u64 first, u64 stride) {
  return col_differ2(d + a, d + b, len, first, stride);
}

__global__ __launch_bounds__(COL_T) void k_col_flags(const u64 *lt, u64 L, u32 *flag, u64 *ctl) {
  const u64 i = (u64)blockIdx.x * COL_T + threadIdx.x;
  if (i < COL_CTL_WORDS) ctl[i] = i == COL_BAD ? ~0ull : 0ull;
  if (i < L) flag[i] = lt[2 * i + 1] > 1 ? 1u : 0u;
}

__global__ __launch_bounds__(COL_T) void k_col_keys(const uint8_t *d, u64 n, const u64 *lt, u64 L, u32 c,
                                                    const u32 *flag, const u64 *rank, ColKey *ck, u64 *ctl) {
  const u64 i = (u64)blockIdx.x * COL_T + threadIdx.x;
  if (i >= L) return;
  const u32 f = flag[i];
  const u64 r = rank[i];
  if (f) {
    ColKey k;
    k.off = lt[2 * i];
    if (!col_key(d, n, k.off, lt[2 * i + 1], c, k.lo, k.len)) atomicMin(&ctl[COL_BAD], k.off);
    ck[r] = k;
  }
  if (i == L - 1) ctl[COL_NB] = r + f;
}

// cutf[r] for the non-blank line of rank r (0 at and above the count): column.go:80 with
// prev_str = "" before the first compared line and no cut at line 0 (offset 0)
__global__ __launch_bounds__(COL_T) void k_col_cmp(const uint8_t *d, const ColKey *ck, u64 L, const u64 *ctl,
                                                   u32 *cutf) {
  const u64 r = (u64)blockIdx.x * COL_T + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const u64 nb = ctl[COL_NB];
  u32 cut = 0;
  bool wide = false;
  u64 a = 0, b = 0, len = 0;
  if (r < nb) {
    const ColKey k = ck[r];
    a = k.lo;
    len = k.len;
    if (r == 0) {
      cut = (k.off != 0 && k.len != 0) ? 1u : 0u;
    } else {
      const ColKey p = ck[r - 1];
      b = p.lo;
      if (k.len != p.len) cut = 1;
      else if (k.len > COL_WAVE_KEY) wide = true;
      else cut = col_differ(d, a, b, len, 0, 16) ? 1u : 0u;
    }
  }
  for (u64 w = __ballot(wide); w; w &= w - 1) {  // (every lane of the wave is here)
    const int src = (int)ctz64(w);
    const u64 wa = __shfl(a, src, 64), wb = __shfl(b, src, 64), wl = __shfl(len, src, 64);
    const bool df = col_differ(d, wa, wb, wl, (u64)lane * 16, 1024);
    if (__ballot(df) && lane == src) cut = 1;
  }
  if (r < L) cutf[r] = cut;
}

__global__ __launch_bounds__(COL_T) void k_col_cuts(const ColKey *ck, const u32 *cutf, const u64 *cpos, u64 L,
                                                    u64 *cuts, u64 *ctl) {
  const u64 r = (u64)blockIdx.x * COL_T + threadIdx.x;
  if (r >= L) return;
  const u32 f = cutf[r];
  const u64 k = cpos[r];
  if (f) cuts[k] = ck[r].off;
  if (r == L - 1) ctl[COL_B] = k + f;
}

// column.go:90-96,119-125: rows between adjacent cut points 0, cuts..., n; none without a cut
__global__ __launch_bounds__(COL_T) void k_col_rows(const u64 *cuts, const u64 *ctl, u64 n, u64 *rows, u64 row_cap) {
  const u64 k = (u64)blockIdx.x * COL_T + threadIdx.x;
  const u64 B = ctl[COL_B];
  if (!B || k > B || k >= row_cap) return;
  const u64 p0 = k ? cuts[k - 1] : 0, p1 = k < B ? cuts[k] : n;
  reinterpret_cast<ulonglong2 *>(rows)[k] = make_ulonglong2(p0, p1 - p0);
}

// the DevResult k_verify_rows reads, and the one invariant it does not cover
__global__ void k_col_check(const u64 *rows, u64 count, u64 n, DevResult *res) {
  if (threadIdx.x != 0) return;
  DevResult r = {};
  r.count = count;
  if (count && rows[2 * (count - 1)] + rows[2 * (count - 1) + 1] != n) r.flags = RF_INTERNAL;
  if (count && rows[0] != 0) r.flags = RF_INTERNAL;
  *res = r;
}

// ====================================================================================
// The tile pass
// ====================================================================================
constexpr u32 CT_NONE = 0xFFFFu;     // a tile word's line field: none
constexpr u64 CT_NOKEY = ~0ull;      // a thread without a non-blank line
constexpr u32 COL_CSLOT = TILE / 2;  // u16 cut entries per tile (a compared line has >= 2 bytes in it)
// the tile word: decided cuts | first undecided line << 16 | the line past the end << 32 | that
// line's predecessor << 48 (tile-relative line starts, CT_NONE: none)
__device__ __forceinline__ u64 ct_word(u32 cnt, u32 d0, u32 d1, u32 d1p) {
  return (u64)cnt | ((u64)d0 << 16) | ((u64)d1 << 32) | ((u64)d1p << 48);
}

// col_key over the tile's '\t' mask words in LDS: the line at tile-relative [s, e)
__device__ bool col_key_lds(const u64 *stab, u32 s, u32 e, u32 c, u32 &lo, u32 &klen) {
  u32 t = 0;
  lo = s;
  for (u32 w = s >> 6; (w << 6) < e; ++w) {
    u64 m = stab[w];
    if ((w << 6) < s) m &= ~0ull << (s & 63);
    if ((w << 6) + 64 > e) m &= lowmask(e - (w << 6));
    const u32 pc = popc64(m);
    if (t + pc + 1 < c) {
      t += pc;
      continue;
    }
    while (m) {
      const u32 pos = (w << 6) + ctz64(m);
      m &= m - 1;
      if (++t == c) {
        klen = pos - lo;
        return true;
      }
      if (t + 1 == c) lo = pos + 1;
    }
  }
  if (t + 1 < c) {
    klen = 0;
    return false;
  }
  klen = e - lo;
  return true;
}

// 8 bytes of the tile at any tile-relative position: three aligned dwords, two byte alignments
// (the slot is padded so the dwords past a key's end exist)
__device__ __forceinline__ u64 lds_get64(const uint8_t *tb, u32 pos) {
  const u32 *w = reinterpret_cast<const u32 *>(tb) + (pos >> 2);
  const u32 w0 = w[0], w1 = w[1], w2 = w[2], sh = pos & 3u;
  return (u64)__builtin_amdgcn_alignbyte(w1, w0, sh) | ((u64)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32);
}
__device__ bool col_differ_lds(const uint8_t *tb, u32 a, u32 b, u32 len) {
  for (u32 i = 0; i < len; i += 8) {
    u64 x = lds_get64(tb, a + i) ^ lds_get64(tb, b + i);
    if (len - i < 8) x &= lowmask(8 * (len - i));
    if (x) return true;
  }
  return false;
}

#ifndef SIDX_COL_WGS
#define SIDX_COL_WGS 7  // workgroups per CU, as k_line_tiles (22.6 KiB of LDS each)
#endif
__global__ __launch_bounds__(SNT, SIDX_COL_WGS) void k_col_tiles(const SlabParams p, u32 c, u64 *tword, u64 *plast,
                                                                 uint16_t *cslot, u64 *ctl) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[FRONT + TILE + 16];  // (+ 16: lds_get64 reads whole dwords)
  __shared__ u64 snl[SNT], stab[SNT];  // '\n' / '\t' masks of each thread's 64 bytes
  __shared__ u64 tl[SNT];              // each thread's last non-blank line: start | key lo << 16 | key length << 32
  __shared__ u32 wtot[SNW], wlast[SNW], sD[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const u64 G = p.pgrid;
  const uint8_t *tb = raw + FRONT;
  const u64 fend = (p.eof && p.n == p.end) ? p.n : ~0ull;  // where the owned bytes end the file (a slab's may not)
  const u64 flast = p.eof ? p.end - 1 : ~0ull;             // the file's last byte, if the slab can read it
  for (u64 t = first_tile(blockIdx.x, G); t < p.ntiles; t += G) {
    stage_tile<false>(p, t, (u32)(size_t)(lds_u8 *)raw, wid, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const u64 tlo = t * TILE;
    const u32 tlen = (u32)(((tlo + TILE < p.n) ? tlo + TILE : p.n) - tlo);
    // the tile ends the file (a slab whose owned bytes stop before the file does has no such tile:
    // the lines that leave its last tile end in its halo, or later)
    const bool last_tile = tlo + tlen == fend;
    u64 mnl = 0, mtb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32 cj = ((u32)j + ((u32)tid >> 2)) & 3u;
      const uint4 v = *reinterpret_cast<const uint4 *>(tb + tid * 64 + 16 * cj);
      mnl |= (u64)eq16x(v, '\n') << (16 * cj);
      mtb |= (u64)eq16x(v, '\t') << (16 * cj);
    }
    if (eq_suspect(mnl) || eq_suspect(mtb)) {  // "\n\v" or "\t\b" inside a dword: the exact masks
      mnl = mtb = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint4 v = *reinterpret_cast<const uint4 *>(tb + tid * 64 + 16 * j);
        mnl |= (u64)eq16(v, '\n') << (16 * j);
        mtb |= (u64)eq16(v, '\t') << (16 * j);
      }
    }
    const u32 rl = tlen > (u32)tid * 64 ? tlen - (u32)tid * 64 : 0u;
    mnl &= lowmask(rl);  // bytes past the end were zero-filled or are not this tile's
    mtb &= lowmask(rl);
    tail_bytes(p, tlo, tlen, tid, [&](uint8_t ch, u32 bit) {  // the DMA left the last partial dword zero
      mnl |= (u64)(ch == '\n') << bit;
      mtb |= (u64)(ch == '\t') << bit;
      raw[FRONT + tid * 64 + bit] = ch;
    });
    snl[tid] = mnl;
    stab[tid] = mtb;
    if (tid < 3) sD[tid] = CT_NONE;
    lds_barrier();
    // ---- this thread's lines: the one after each of its '\n's (thread 0 of tile 0: line 0 first)
    const u32 nw = (tlen + 63) >> 6;
    u64 cutm = 0;                            // its '\n's whose line is a decided cut
    u32 fS = CT_NONE, fLo = 0, fLen = 0;     // its first non-blank line: the compare waits for a predecessor
    int fBit = 0;
    u32 pS = CT_NONE, pLo = 0, pLen = 0;     // its last non-blank line so far
    u32 xS = CT_NONE;                        // the non-blank line that runs past the tile (one thread)
    auto do_line = [&](u32 s, int bit) {
      u32 e = 0;
      bool found = false;
      if (s < tlen) {
        u32 w = s >> 6;
        u64 m = snl[w] & (~0ull << (s & 63));
        for (;;) {
          if (m) {
            e = (w << 6) + ctz64(m) + 1;
            found = true;
            break;
          }
          if (++w >= nw) break;
          m = snl[w];
        }
      }
      if (!found) {
        if (!last_tile) {  // it ends in a later tile: blank only if it starts there with "\n" or as the file's last byte
          // (a slab without a readable byte there cannot tell: the line goes to k_col_fix, which reports it)
          const u64 a = tlo + tlen;
          if (s < tlen || a >= p.end || (p.data[a] != '\n' && a != flast)) xS = s;
          return;
        }
        e = tlen;  // the file's last piece
      }
      if (e - s <= 1) return;  // blank (column.go:64)
      u32 lo, klen;
      if (!col_key_lds(stab, s, e, c, lo, klen)) atomicMin(&ctl[COL_BAD], tlo + s);
      if (pS != CT_NONE) {
        if (klen != pLen || col_differ_lds(tb, lo, pLo, klen)) cutm |= 1ull << bit;
      } else {
        fS = s;
        fLo = lo;
        fLen = klen;
        fBit = bit;
      }
      pS = s;
      pLo = lo;
      pLen = klen;
    };
    if (t == 0 && tid == 0 && p.file_start) do_line(0, -1);
    for (u64 b = mnl; b; b &= b - 1) {
      const int bit = (int)ctz64(b);
      do_line((u32)tid * 64 + (u32)bit + 1, bit);
    }
    tl[tid] = pS == CT_NONE ? CT_NOKEY : ((u64)pS | ((u64)pLo << 16) | ((u64)pLen << 32));
    lds_barrier();
    // ---- the predecessor of a thread's first line is an earlier thread's last
    if (fS != CT_NONE || (xS != CT_NONE && pS == CT_NONE)) {
      u64 q = CT_NOKEY;
      for (int k = tid - 1; k >= 0 && q == CT_NOKEY; --k) q = tl[k];
      if (fS != CT_NONE) {
        if (q == CT_NOKEY) sD[0] = fS;  // the tile's first non-blank line
        else if (fLen != (u32)(q >> 32) || col_differ_lds(tb, fLo, (u32)(q >> 16) & 0xFFFFu, fLen)) cutm |= 1ull << fBit;
      } else if (q == CT_NOKEY) {
        sD[0] = xS;
      } else {
        sD[1] = xS;
        sD[2] = (u32)q & 0xFFFFu;
      }
    }
    if (xS != CT_NONE && pS != CT_NONE) {
      sD[1] = xS;
      sD[2] = pS;
    }
    const u32 cc = popc64(cutm);
    const u32 incl = wave_scan_add(cc);
    const u32 mine = xS != CT_NONE ? xS + 1 : (pS != CT_NONE ? pS + 1 : 0u);  // its last non-blank line + 1
    const u64 lb = __ballot(mine != 0);
    const u32 lmx = lb ? (u32)__builtin_amdgcn_readlane((int)mine, 63 - (int)clz64(lb)) : 0u;
    if (lane == 63) {
      wtot[wid] = incl;
      wlast[wid] = lmx;
    }
    lds_barrier();
    u32 wpre = 0, T = 0, L = 0;
#pragma unroll
    for (int w = 0; w < SNW; ++w) {
      const u32 x = wtot[w];
      if (w < wid) wpre += x;
      T += x;
      if (wlast[w]) L = wlast[w];
    }
    u32 o = wpre + incl - cc;
    for (u64 b = cutm; b; b &= b - 1) cslot[t * COL_CSLOT + o++] = (uint16_t)((u32)tid * 64 + ctz64(b) + 1);
    if (tid == 0) {
      tword[t] = ct_word(T, sD[0], sD[1], sD[2]);
      plast[t] = L ? tlo + L : 0ull;
    }
    lds_barrier();  // raw, the masks and sD are rewritten by the next tile
  }
}

// col_key for the line that starts at s, its end not known: the scan stops at the line's '\n'
// kWin: d[n) is where a slab's readable bytes end, the file's end only with eof; a line that reaches
// it with neither its key's closing '\t' nor its '\n' is CK_OPEN (the slab cannot settle it)
enum ColKeyState : u32 { CK_OK = 0, CK_BAD = 1, CK_OPEN = 2 };
template <bool kWin>
__device__ u32 col_key_scan(const uint8_t *d, u64 n, bool eof, u64 s, u32 c, u64 &lo, u64 &klen) {
  u64 t = 0, end = n;
  bool closed = false;
  lo = s;
  for (u64 a = s & ~15ull; a < end; a += 16) {
    const uint4 v = col_load16(d, a, n);
    u32 m = eq16(v, '\t'), ml = eq16(v, '\n');
    if (a < s) {
      m &= ~0u << (u32)(s - a);
      ml &= ~0u << (u32)(s - a);
    }
    if (ml) {  // the line ends here: tabs up to its '\n' only
      end = a + (u32)__builtin_ctz(ml) + 1;
      m &= (1u << (u32)(end - a)) - 1u;
      closed = true;
    }
    while (m) {
      const u64 pos = a + (u32)__builtin_ctz(m);
      m &= m - 1;
      if (++t == c) {
        klen = pos - lo;
        return CK_OK;
      }
      if (t + 1 == c) lo = pos + 1;
    }
  }
  klen = 0;
  if (kWin && !closed && !eof) return CK_OPEN;
  if (t + 1 < c) return CK_BAD;
  klen = end - lo;
  return CK_OK;
}
__device__ bool col_key_open(const uint8_t *d, u64 n, u64 s, u32 c, u64 &lo, u64 &klen) {
  return col_key_scan<false>(d, n, true, s, c, lo, klen) == CK_OK;
}

// thread 2 t + j: undecided line j of tile t against its predecessor (j = 0: the last non-blank
// line before the tile, pprev; none: prev_str is "" and line 0 never cuts), from global memory
// kSlab: d[n) is where the slab's readable bytes end (sa.eof: the file's); a line whose key does
// not close before it is reported in COLS_MORE; offsets are the slab's, sa.base the file's of d[0];
// and a tile's first line without a predecessor in the slab is compared with the carried key
// (none carried yet: prev_str is "", and the line at file offset 0 never cuts)
template <bool kSlab>
__global__ __launch_bounds__(COL_T) void k_col_fix(const uint8_t *d, u64 n, u64 ntiles, u32 c, const u64 *tword,
                                                   const u64 *pprev, u32 *fcut, u32 *tot, u64 *ctl,
                                                   const ColSlabArgs sa) {
  const u64 i = (u64)blockIdx.x * COL_T + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const u64 t = i >> 1;
  const u32 j = (u32)i & 1u;
  const bool valid = t < ntiles;
  const u64 w = valid ? tword[t] : ~0ull;
  const u32 ds = (u32)(w >> (j ? 32 : 16)) & 0xFFFFu;
  u32 cut = 0;
  bool wide = false;
  u64 a = 0, b = 0, len = 0;
  const uint8_t *pb = d;  // the predecessor's key is pb[b ..)
  if (valid && ds != CT_NONE) {
    const u64 tlo = t * TILE, s = tlo + ds;
    const u64 pp = j ? tlo + ((u32)(w >> 48) & 0xFFFFu) + 1 : pprev[t];  // predecessor start + 1, 0: none
    u64 plen = 0;
    bool have = pp != 0;
    if (kSlab) {
      const u32 st = col_key_scan<true>(d, n, sa.eof != 0, s, c, a, len);
      if (st == CK_BAD) atomicMin(&ctl[COL_BAD], s);
      if (st == CK_OPEN) atomicMin(&ctl[COLS_MORE], s);
      if (pp) {
        (void)col_key_scan<true>(d, n, sa.eof != 0, pp - 1, c, b, plen);
      } else if (!sa.first) {
        const ColCarryHalf *h = &sa.carry->half[sa.carry->cur & 1];
        if (h->seen) {
          have = true;
          pb = h->key;
          plen = h->klen;
        }
      }
    } else {
      if (!col_key_open(d, n, s, c, a, len)) atomicMin(&ctl[COL_BAD], s);
      if (pp) (void)col_key_open(d, n, pp - 1, c, b, plen);
    }
    if (!have) cut = ((kSlab ? sa.base + s : s) != 0 && len != 0) ? 1u : 0u;
    else if (len != plen) cut = 1;
    else if (len > COL_WAVE_KEY) wide = true;
    else cut = col_differ2(d + a, pb + b, len, 0, 16) ? 1u : 0u;
  }
  for (u64 wm = __ballot(wide); wm; wm &= wm - 1) {  // (every lane of the wave is here)
    const int src = (int)ctz64(wm);
    const u64 wa = __shfl((u64)(d + a), src, 64), wb = __shfl((u64)(pb + b), src, 64), wl = __shfl(len, src, 64);
    const bool df = col_differ2((const uint8_t *)wa, (const uint8_t *)wb, wl, (u64)lane * 16, 1024);
    if (__ballot(df) && lane == src) cut = 1;
  }
  const u32 other = (u32)__shfl_xor((int)cut, 1, 64);
  if (valid) {
    fcut[i] = cut;
    if (!j) tot[t] = ((u32)w & 0xFFFFu) + cut + other;
  }
}

__global__ void k_col_init(u64 *ctl) {
  if (threadIdx.x < COL_CTL_WORDS) ctl[threadIdx.x] = threadIdx.x == COL_BAD ? ~0ull : 0ull;
}
__global__ void k_col_total(const u64 *cbase, const u32 *tot, u64 ntiles, u64 *ctl) {
  if (threadIdx.x == 0) ctl[COL_B] = cbase[ntiles - 1] + tot[ntiles - 1];
}

// one wave per tile: the offsets of its cuts (the first undecided line, the decided ones, the
// line past its end, in file order) into the rows they start: cut k starts row k + 1
__global__ __launch_bounds__(COL_T) void k_col_place(u64 ntiles, const u64 *tword, const u32 *fcut, const u64 *cbase,
                                                     const uint16_t *cslot, u64 *rows, u64 row_cap) {
  const u64 t = ((u64)blockIdx.x * COL_T + threadIdx.x) >> 6;
  const u32 lane = threadIdx.x & 63;
  if (t >= ntiles) return;
  const u64 w = tword[t], tlo = t * TILE, base = cbase[t];
  const u32 cnt = (u32)w & 0xFFFFu, f0 = fcut[2 * t], f1 = fcut[2 * t + 1];
  auto put = [&](u64 k, u64 off) {
    if (k + 1 < row_cap) rows[2 * (k + 1)] = off;
  };
  if (lane == 0 && f0) put(base, tlo + ((u32)(w >> 16) & 0xFFFFu));
  for (u32 j = lane; j < cnt; j += 64) put(base + f0 + j, tlo + cslot[t * COL_CSLOT + j]);
  if (lane == 0 && f1) put(base + f0 + cnt, tlo + ((u32)(w >> 32) & 0xFFFFu));
}

__global__ __launch_bounds__(COL_T) void k_col_lens(u64 *rows, u64 count, u64 n) {
  const u64 k = (u64)blockIdx.x * COL_T + threadIdx.x;
  if (k >= count) return;
  const u64 off = k ? rows[2 * k] : 0, next = k + 1 < count ? rows[2 * (k + 1)] : n;
  if (!k) rows[0] = 0;
  rows[2 * k + 1] = next - off;
}

// ====================================================================================
// The slab pass: the tile pass over one slab of the file, column.go's loop state carried in
// ====================================================================================
__device__ __forceinline__ const ColCarryHalf *col_carry_in(const ColSlabArgs &sa) {
  return sa.first ? nullptr : &sa.carry->half[sa.carry->cur & 1];
}

__global__ void k_col_slab_init(u64 *ctl) {
  if (threadIdx.x < COL_SLAB_WORDS) ctl[threadIdx.x] = (threadIdx.x == COL_BAD || threadIdx.x == COLS_MORE) ? ~0ull : 0ull;
}

// After the cut scan, one thread: the slab's cuts, its last non-blank owned line and that line's
// key (what the next slab compares its first line with; longer than a carry holds: the slab
// cannot settle it, unless no slab follows), and the rows it writes -- one per cut, and in the
// file's last slab the row that runs to the file's end when the file has a cut (column.go:119-125)
__global__ void k_col_slab_sum(const uint8_t *d, const ColSlabArgs sa, u64 ntiles, u32 c, const u64 *cbase,
                               const u32 *tot, const u64 *pprev, const u64 *plast, u64 *ctl) {
  if (threadIdx.x != 0) return;
  u64 B = 0, L = 0, klo = 0, klen = 0;
  if (ntiles) {
    B = cbase[ntiles - 1] + tot[ntiles - 1];
    const u64 x = pprev[ntiles - 1], y = plast[ntiles - 1];
    L = x > y ? x : y;
  }
  if (L && ctl[COL_BAD] == ~0ull && ctl[COLS_MORE] == ~0ull) {
    const u32 st = col_key_scan<true>(d, sa.end, sa.eof != 0, L - 1, c, klo, klen);
    if (st != CK_OK || (klen > COL_KEYCAP && !sa.last)) ctl[COLS_MORE] = L - 1;
  }
  const ColCarryHalf *h = col_carry_in(sa);
  const u64 before = h ? h->rows : 0;
  ctl[COL_B] = B;
  ctl[COLS_LAST] = L;
  ctl[COLS_KLO] = klo;
  ctl[COLS_KLEN] = klen;
  ctl[COLS_ROWS] = B + ((sa.last && before + B) ? 1u : 0u);
}

// one wave per tile, as k_col_place: cut k of the slab ends row k and starts row k + 1 (file offsets)
__global__ __launch_bounds__(COL_T) void k_col_slab_place(u64 ntiles, u64 base, const u64 *tword, const u32 *fcut,
                                                          const u64 *cbase, const uint16_t *cslot, u64 *rows,
                                                          u64 nrows) {
  const u64 t = ((u64)blockIdx.x * COL_T + threadIdx.x) >> 6;
  const u32 lane = threadIdx.x & 63;
  if (t >= ntiles) return;
  const u64 w = tword[t], tlo = base + t * TILE, cb = cbase[t];
  const u32 cnt = (u32)w & 0xFFFFu, f0 = fcut[2 * t], f1 = fcut[2 * t + 1];
  auto put = [&](u64 k, u64 off) {
    if (k < nrows) rows[2 * k + 1] = off;
    if (k + 1 < nrows) rows[2 * (k + 1)] = off;
  };
  if (lane == 0 && f0) put(cb, tlo + ((u32)(w >> 16) & 0xFFFFu));
  for (u32 j = lane; j < cnt; j += 64) put(cb + f0 + j, tlo + cslot[t * COL_CSLOT + j]);
  if (lane == 0 && f1) put(cb + f0 + cnt, tlo + ((u32)(w >> 32) & 0xFFFFu));
}

// row k of the slab from the ends k_col_slab_place left: it starts at the cut before it (row 0:
// the carried one) and ends at its cut (the row after the slab's last cut: at the file's end)
__global__ __launch_bounds__(COL_T) void k_col_slab_close(const ColSlabArgs sa, const u64 *ctl, u64 *rows, u64 nrows) {
  const u64 k = (u64)blockIdx.x * COL_T + threadIdx.x;
  if (k >= nrows) return;
  const ColCarryHalf *h = col_carry_in(sa);
  const u64 off = k ? rows[2 * k] : (h ? h->prev_cut : 0ull);
  const u64 end = k < ctl[COL_B] ? rows[2 * k + 1] : sa.file_size;
  reinterpret_cast<ulonglong2 *>(rows)[k] = make_ulonglong2(off, end - off);
}

// The carry after the slab, into the half the slab did not read; then that half becomes current.
// One workgroup: the key of the slab's last non-blank owned line (none: the carried one again).
__global__ __launch_bounds__(COL_T) void k_col_slab_carry(const uint8_t *d, const ColSlabArgs sa, ColCarry *carry,
                                                          const u64 *ctl, const u64 *rows, u64 nrows) {
  const u32 cur = sa.first ? 1u : (u32)(carry->cur & 1);
  const ColCarryHalf *h = col_carry_in(sa);
  ColCarryHalf *o = &carry->half[cur ^ 1u];
  const u64 B = ctl[COL_B], L = ctl[COLS_LAST];
  const uint8_t *src = L ? d + ctl[COLS_KLO] : (h ? h->key : d);
  u64 klen = L ? ctl[COLS_KLEN] : (h && h->seen ? h->klen : 0ull);
  if (klen > COL_KEYCAP) klen = COL_KEYCAP;  // (the file's last slab: nothing reads this carry)
  for (u64 i = threadIdx.x; i < klen; i += COL_T) o->key[i] = src[i];
  if (threadIdx.x == 0) {
    o->prev_cut = B ? rows[2 * (B - 1)] + rows[2 * (B - 1) + 1] : (h ? h->prev_cut : 0ull);
    o->rows = (h ? h->rows : 0ull) + nrows;
    o->seen = (L || (h && h->seen)) ? 1ull : 0ull;
    o->klen = klen;
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) carry->cur = cur ^ 1u;
}

}  // namespace sidx

using namespace sidx;

namespace {
inline u32 nblk(u64 n) { return (u32)((n + COL_T - 1) / COL_T); }
}  // namespace

extern "C" u64 sidx_col_scan_bytes(u64 L) {
  size_t sb = 0;
  (void)sidx_scan_flags(nullptr, nullptr, L ? L : 1, nullptr, &sb, nullptr);
  return sb;
}

// The general build up to the cut count: lt = the line index of d (L >= 1 rows, overwritten with
// the cut offsets), flag / rank / ck = L entries each, ctl = COL_CTL_WORDS words (left holding
// the first bad line's offset, the non-blank lines and the cuts).
extern "C" hipError_t sidx_col_cuts(const uint8_t *d, u64 n, u64 *lt, u64 L, u32 column, u32 *flag, u64 *rank,
                                    ColKey *ck, u64 *ctl, void *scan_tmp, size_t scan_bytes, hipStream_t s) {
  const u32 g = nblk(L);
  hipLaunchKernelGGL(k_col_flags, dim3(g), dim3(COL_T), 0, s, lt, L, flag, ctl);
  hipError_t e = sidx_scan_flags(flag, rank, L, scan_tmp, &scan_bytes, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_col_keys, dim3(g), dim3(COL_T), 0, s, d, n, lt, L, column, flag, rank, ck, ctl);
  hipLaunchKernelGGL(k_col_cmp, dim3(g), dim3(COL_T), 0, s, d, ck, L, ctl, flag);
  e = sidx_scan_flags(flag, rank, L, scan_tmp, &scan_bytes, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_col_cuts, dim3(g), dim3(COL_T), 0, s, ck, flag, rank, L, lt, ctl);
  return hipGetLastError();
}

// the B + 1 rows from the B >= 1 cut offsets (those that fit row_cap)
extern "C" hipError_t sidx_col_rows(const u64 *cuts, const u64 *ctl, u64 B, u64 n, u64 *rows, u64 row_cap,
                                    hipStream_t s) {
  hipLaunchKernelGGL(k_col_rows, dim3(nblk(B + 1)), dim3(COL_T), 0, s, cuts, ctl, n, rows, row_cap);
  return hipGetLastError();
}

extern "C" hipError_t sidx_col_check(const u64 *rows, u64 count, u64 n, DevResult *d_res, hipStream_t s) {
  hipLaunchKernelGGL(k_col_check, dim3(1), dim3(64), 0, s, rows, count, n, d_res);
  return hipGetLastError();
}

// ---- the tile pass -------------------------------------------------------------------
namespace {
struct ColTileWs {  // carved from one workspace of sidx_col_tile_bytes(ntiles) bytes
  u64 *ctl, *tword, *plast, *pprev, *cbase;
  u32 *fcut, *tot;
  uint16_t *cslot;
  void *scan_tmp;
  size_t scan_bytes;
};
inline u64 r256(u64 b) { return (b + 255) & ~255ull; }
size_t col_tile_scan_bytes(u64 nt) {
  size_t a = 0, b = 0;
  (void)dscan::run<u64, dscan::Max, true>(nullptr, &a, (const u64 *)nullptr, nullptr, nt, nullptr);
  (void)dscan::run<u32, dscan::Sum, true>(nullptr, &b, (const u32 *)nullptr, nullptr, nt, nullptr);
  return a > b ? a : b;
}
ColTileWs col_tile_carve(void *ws, u64 nt) {
  uint8_t *q = (uint8_t *)ws;
  auto take = [&](u64 bytes) { uint8_t *r = q; q += r256(bytes); return r; };
  ColTileWs w;
  w.ctl = (u64 *)take(8 * COL_CTL_WORDS);
  w.tword = (u64 *)take(8 * nt);
  w.plast = (u64 *)take(8 * nt);
  w.pprev = (u64 *)take(8 * nt);
  w.cbase = (u64 *)take(8 * nt);
  w.fcut = (u32 *)take(8 * nt);
  w.tot = (u32 *)take(4 * nt);
  w.scan_bytes = col_tile_scan_bytes(nt);
  w.scan_tmp = take(w.scan_bytes);
  w.cslot = (uint16_t *)take(2ull * COL_CSLOT * nt);
  return w;
}
}  // namespace

extern "C" u64 sidx_col_tile_bytes(u64 ntiles) {
  return 256 + 5 * r256(8 * ntiles) + r256(4 * ntiles) + r256(col_tile_scan_bytes(ntiles)) + r256(2ull * COL_CSLOT * ntiles);
}

// The tile pass up to the cut count (n > 0): *ctl_out = the control words in ws (left holding the
// first bad line's offset and the cuts).  grid: the persistent grid of the tile passes.
extern "C" hipError_t sidx_col_tile_cuts(const uint8_t *d, u64 n, u32 column, u32 grid, void *ws, const u64 **ctl_out,
                                         hipStream_t s) {
  const u64 nt = (n + TILE - 1) / TILE;
  const ColTileWs w = col_tile_carve(ws, nt);
  *ctl_out = w.ctl;
  SlabParams p;
  memset(&p, 0, sizeof p);
  p.data = d;
  p.n = p.end = n;
  p.ntiles = (u32)nt;
  p.pgrid = grid && grid < nt ? grid : (u32)nt;
  p.eof = p.file_start = 1;
  hipLaunchKernelGGL(k_col_init, dim3(1), dim3(64), 0, s, w.ctl);
  hipLaunchKernelGGL(k_col_tiles, dim3(p.pgrid), dim3(SNT), 0, s, p, column, w.tword, w.plast, w.cslot, w.ctl);
  size_t sb = w.scan_bytes;
  hipError_t e = dscan::run<u64, dscan::Max, true>(w.scan_tmp, &sb, (const u64 *)w.plast, w.pprev, nt, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_col_fix<false>, dim3(nblk(2 * nt)), dim3(COL_T), 0, s, d, n, nt, column, w.tword, w.pprev, w.fcut,
                     w.tot, w.ctl, ColSlabArgs{});
  e = dscan::run<u32, dscan::Sum, true>(w.scan_tmp, &sb, (const u32 *)w.tot, w.cbase, nt, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_col_total, dim3(1), dim3(64), 0, s, w.cbase, w.tot, nt, w.ctl);
  return hipGetLastError();
}

// the count = cuts + 1 rows (count <= row_cap) from the tile pass's workspace
extern "C" hipError_t sidx_col_tile_rows(u64 n, void *ws, u64 count, u64 *rows, u64 row_cap, hipStream_t s) {
  const u64 nt = (n + TILE - 1) / TILE;
  const ColTileWs w = col_tile_carve(ws, nt);
  hipLaunchKernelGGL(k_col_place, dim3(nblk(64 * nt)), dim3(COL_T), 0, s, nt, w.tword, w.fcut, w.cbase, w.cslot, rows,
                     row_cap);
  hipLaunchKernelGGL(k_col_lens, dim3(nblk(count)), dim3(COL_T), 0, s, rows, count, n);
  return hipGetLastError();
}

// ---- the slab pass -------------------------------------------------------------------
// One slab up to its host stop (sl: the slab, sa.carry: the carry it reads): *ctl_out = the
// COL_SLAB_WORDS control words in ws (sidx_col_tile_bytes(tiles of sl.n) bytes).
extern "C" hipError_t sidx_col_slab_cuts(const uint8_t *d, u64 n, u64 front, const ColSlabArgs *sa, u32 column, u32 grid,
                                         void *ws, const u64 **ctl_out, hipStream_t s) {
  const u64 nt = (n + TILE - 1) / TILE;
  const ColTileWs w = col_tile_carve(ws, nt ? nt : 1);
  *ctl_out = w.ctl;
  hipLaunchKernelGGL(k_col_slab_init, dim3(1), dim3(64), 0, s, w.ctl);
  if (nt) {
    SlabParams p;
    memset(&p, 0, sizeof p);
    p.data = d;
    p.n = n;
    p.end = sa->end;
    p.front = front;
    p.base = sa->base;
    p.ntiles = (u32)nt;
    p.pgrid = grid && grid < nt ? grid : (u32)nt;
    p.eof = sa->eof;
    p.file_start = sa->first;
    hipLaunchKernelGGL(k_col_tiles, dim3(p.pgrid), dim3(SNT), 0, s, p, column, w.tword, w.plast, w.cslot, w.ctl);
    size_t sb = w.scan_bytes;
    hipError_t e = dscan::run<u64, dscan::Max, true>(w.scan_tmp, &sb, (const u64 *)w.plast, w.pprev, nt, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_col_fix<true>, dim3(nblk(2 * nt)), dim3(COL_T), 0, s, d, sa->end, nt, column, w.tword, w.pprev,
                       w.fcut, w.tot, w.ctl, *sa);
    e = dscan::run<u32, dscan::Sum, true>(w.scan_tmp, &sb, (const u32 *)w.tot, w.cbase, nt, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_col_slab_sum, dim3(1), dim3(64), 0, s, d, *sa, nt, column, w.cbase, w.tot, w.pprev, w.plast, w.ctl);
  return hipGetLastError();
}

// the slab's nrows rows (nrows <= the capacity of rows) and the carry after it
extern "C" hipError_t sidx_col_slab_rows(const uint8_t *d, u64 n, const ColSlabArgs *sa, void *ws, ColCarry *carry,
                                         u64 *rows, u64 nrows, hipStream_t s) {
  const u64 nt = (n + TILE - 1) / TILE;
  const ColTileWs w = col_tile_carve(ws, nt ? nt : 1);
  if (nrows) {
    if (nt)
      hipLaunchKernelGGL(k_col_slab_place, dim3(nblk(64 * nt)), dim3(COL_T), 0, s, nt, sa->base, w.tword, w.fcut, w.cbase,
                         w.cslot, rows, nrows);
    hipLaunchKernelGGL(k_col_slab_close, dim3(nblk(nrows)), dim3(COL_T), 0, s, *sa, w.ctl, rows, nrows);
  }
  hipLaunchKernelGGL(k_col_slab_carry, dim3(1), dim3(COL_T), 0, s, d, *sa, carry, w.ctl, rows, nrows);
  return hipGetLastError();
}
