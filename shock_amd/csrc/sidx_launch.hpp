// sidx_launch.hpp -- every kernel launcher and query that crosses from a .hip file to host code.
//
// Included by the host files that call them and by the .hip file that defines each, so a
// definition that drifts from its prototype is a compile error ("conflicting types"), not
// garbage arguments at run time.  The one declaration of each function in the tree.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sidx_batch.hpp"
#include "sidx_common.hpp"
#include "sidx_subset.hpp"

extern "C" {

hipError_t sidx_launch_detect(const uint8_t *d, sidx::u64 n, int *d_out, hipStream_t s);
// DetermineFormat per section {int64 pos, int64 len} of d (sections checked against n): d_out[s] = the format
hipError_t sidx_launch_detect_sections(const uint8_t *d, sidx::u64 n, const void *d_secs, sidx::u64 nsecs, int *d_out,
    hipStream_t s);
// one slab's build on the given path (the two-pass build's format: p->gate_fmt)
hipError_t sidx_launch_tiles(sidx::TilePass pass, const sidx::SlabParams *p, sidx::DevResult *d_res, hipStream_t s,
    hipEvent_t ek0, hipEvent_t ek1);
// u32 words of SlabParams::tile_stage that path needs (grid: the caller's persistent grid)
sidx::u64 sidx_tile_stage_words(sidx::TilePass pass, sidx::u64 ntiles, sidx::u32 grid);
hipError_t sidx_launch_chunkrecord(const uint8_t *d, sidx::u64 n, int fasta, long long chunk, sidx::u64 *rows,
    sidx::u64 row_cap, sidx::u64 *out, long long curr0, sidx::u64 cnt0, sidx::u64 max_steps, hipStream_t s);
hipError_t sidx_cr_gpos_count(const uint8_t *d, sidx::u64 n, sidx::u64 *tcnt, sidx::u64 *toff, uint16_t *slot,
    void *scan_tmp, size_t *scan_bytes, hipStream_t s);
hipError_t sidx_cr_gpos_write(const uint8_t *d, sidx::u64 n, const sidx::u64 *tcnt, const sidx::u64 *toff,
    const uint16_t *slot, sidx::u64 *G, hipStream_t s);
sidx::u32 sidx_cr_gslot();
hipError_t sidx_cr_graph(const uint8_t *d, sidx::u64 n, int fasta, sidx::u64 chunk, const sidx::u64 *base,
    sidx::u64 stride, sidx::u64 count, sidx::u64 org, sidx::u64 *ft, sidx::u32 *J1, sidx::u32 *Ja, sidx::u32 *Jb,
    int levels, const sidx::u32 **JL, hipStream_t s);
hipError_t sidx_cr_round(const uint8_t *d, sidx::u64 n, int fasta, sidx::u64 chunk, const sidx::u64 *base,
    sidx::u64 stride, sidx::u64 count, sidx::u64 org, const sidx::u64 *ft, const sidx::u32 *JL, const sidx::u32 *J1,
    sidx::u32 L, sidx::u64 y, sidx::u64 k0, sidx::u64 cap, sidx::u32 *heads, sidx::u64 *pos, sidx::i64 *mres,
    sidx::u64 *ctl, sidx::u64 *rows, sidx::u64 row_cap, sidx::u32 verify_grid, int slab, hipStream_t s);
int sidx_cr_verify_blocks_per_cu();
// the chunkrecord slab step (sidx_chunk.hip; the view, the carry and the control words st:
// sidx_common.hpp): the carry into st (the first slab initialises it with fmt); the serial walk over
// the view from st, or from chunk start y with k rows out; the end state into the carry; node 0 of
// a view's position table
hipError_t sidx_cr_slab_begin(const sidx::ChunkView *v, sidx::u64 chunk, int first, int fmt, sidx::ChunkCarry *carry,
    sidx::u64 *st, hipStream_t s);
hipError_t sidx_cr_slab_walk(const sidx::ChunkView *v, int fasta, sidx::u64 chunk, sidx::u64 *st, sidx::u64 *rows,
    sidx::u64 row_cap, sidx::u64 max_steps, int from_args, sidx::u64 y, sidx::u64 k, hipStream_t s);
hipError_t sidx_cr_slab_commit(sidx::ChunkCarry *carry, const sidx::u64 *st, hipStream_t s);
hipError_t sidx_cr_slab_nodes(sidx::u64 *G, sidx::u64 count, sidx::u64 stride, sidx::u64 bias, sidx::u64 curr,
    hipStream_t s);
sidx::u32 sidx_fa_slot();
hipError_t sidx_fa_bnd_count(const uint8_t *d, sidx::u64 n, sidx::u64 *lnl, sidx::u64 *lgt, sidx::u64 *cnl,
    sidx::u64 *cgt, sidx::u64 *tcnt, sidx::u64 *toff, uint16_t *slot, void *tmp, size_t *tmp_bytes, hipStream_t s);
hipError_t sidx_fa_bnd_write(const uint8_t *d, sidx::u64 n, const sidx::u64 *cnl, const sidx::u64 *cgt,
    const sidx::u64 *tcnt, const sidx::u64 *toff, const uint16_t *slot, sidx::u64 *B, hipStream_t s);
hipError_t sidx_fa_anon_spans(const uint8_t *d, sidx::u64 n, const sidx::u64 *B, sidx::u64 bstride, sidx::u64 m,
    sidx::u64 *bspan, sidx::u64 *outlen, sidx::u64 *firstbad, hipStream_t s);
hipError_t sidx_fa_anon_write(const uint8_t *d, sidx::u64 n, const sidx::u64 *bspan, const sidx::u64 *outoff,
    sidx::u64 K, uint8_t *out, hipStream_t s);
hipError_t sidx_sam_anon_spans(const uint8_t *d, sidx::u64 n, const sidx::u64 *rows, sidx::u64 K, sidx::u64 *span,
    sidx::u64 *outlen, sidx::u64 *firstbad, sidx::u64 *firsteof, hipStream_t s);
hipError_t sidx_sam_anon_write(const uint8_t *d, const sidx::u64 *span, const sidx::u64 *outlen,
    const sidx::u64 *outoff, sidx::u64 K, uint8_t *out, sidx::u64 *count, hipStream_t s);
hipError_t sidx_crs_scan(const sidx::u64 *ri, sidx::u64 R, sidx::u64 *len, sidx::u64 *P, void *tmp,
    size_t *scan_bytes, hipStream_t s);
hipError_t sidx_crs_build(const sidx::u64 *P, sidx::u64 R, sidx::u32 *J1, sidx::u32 *Ja, sidx::u32 *Jb, int levels,
    sidx::u32 *heads, sidx::u64 *rows, sidx::u64 row_cap, sidx::u64 *ctl, hipStream_t s);
int sidx_tiles_blocks_per_cu();
hipError_t sidx_launch_slab_guess(const uint8_t *d, sidx::u64 n, sidx::u64 front, int fmt, sidx::u64 *d_out,
    hipStream_t s);
hipError_t sidx_launch_verify_rows(const sidx::u64 *rows, sidx::u64 row_base, sidx::u64 row_cap,
    sidx::DevResult *d_res, hipStream_t s);
hipError_t sidx_launch_slab_combine(const void *d_all, int world, int rank, int fmt, const uint32_t *expect,
    void *d_plan, hipStream_t s);
hipError_t sidx_id_lines(const uint8_t *text, sidx::u64 n, sidx::u32 *cnt, sidx::u64 *base, sidx::u64 *ends,
    void *tmp, size_t *tmp_bytes, hipStream_t s);
hipError_t sidx_subset_parse(const uint8_t *text, const sidx::u64 *ends, sidx::u64 m, sidx::u32 *keep,
    sidx::i64 *val, sidx::u32 *st, hipStream_t s);
hipError_t sidx_scan_flags(const sidx::u32 *in, sidx::u64 *out, sidx::u64 n, void *tmp, size_t *tmp_bytes,
    hipStream_t s);
hipError_t sidx_scan_u64(const sidx::u64 *in, sidx::u64 *out, sidx::u64 n, void *tmp, size_t *tmp_bytes,
    hipStream_t s);
hipError_t sidx_scan_max_u64(const sidx::u64 *in, sidx::u64 *out, sidx::u64 n, void *tmp, size_t *tmp_bytes,
    hipStream_t s);
sidx::u64 sidx_scan_block();
sidx::u64 sidx_scan_small_items();
// column index (sidx_column.hip): the scans' temp bytes for L lines; the build up to the cut
// offsets (written over the line table lt); the rows from them; the SHOCKIDX_VERIFY end check
sidx::u64 sidx_col_scan_bytes(sidx::u64 L);
hipError_t sidx_col_cuts(const uint8_t *d, sidx::u64 n, sidx::u64 *lt, sidx::u64 L, sidx::u32 column,
    sidx::u32 *flag, sidx::u64 *rank, sidx::ColKey *ck, sidx::u64 *ctl, void *scan_tmp, size_t scan_bytes,
    hipStream_t s);
hipError_t sidx_col_rows(const sidx::u64 *cuts, const sidx::u64 *ctl, sidx::u64 B, sidx::u64 n, sidx::u64 *rows,
    sidx::u64 row_cap, hipStream_t s);
// the tile pass: its workspace bytes; up to the cut count (*ctl: the control words inside ws);
// the count rows from the workspace
sidx::u64 sidx_col_tile_bytes(sidx::u64 ntiles);
hipError_t sidx_col_tile_cuts(const uint8_t *d, sidx::u64 n, sidx::u32 column, sidx::u32 grid, void *ws,
    const sidx::u64 **ctl, hipStream_t s);
hipError_t sidx_col_tile_rows(sidx::u64 n, void *ws, sidx::u64 count, sidx::u64 *rows, sidx::u64 row_cap,
    hipStream_t s);
hipError_t sidx_col_check(const sidx::u64 *rows, sidx::u64 count, sidx::u64 n, sidx::DevResult *d_res,
    hipStream_t s);
// the slab pass: one slab (n owned bytes at d, `front` readable before it) up to its host stop
// (*ctl: the COL_SLAB_WORDS control words inside ws, sidx_col_tile_bytes of the slab's tiles);
// then its nrows rows and the carry after it
hipError_t sidx_col_slab_cuts(const uint8_t *d, sidx::u64 n, sidx::u64 front, const sidx::ColSlabArgs *sa,
    sidx::u32 column, sidx::u32 grid, void *ws, const sidx::u64 **ctl, hipStream_t s);
hipError_t sidx_col_slab_rows(const uint8_t *d, sidx::u64 n, const sidx::ColSlabArgs *sa, void *ws,
    sidx::ColCarry *carry, sidx::u64 *rows, sidx::u64 nrows, hipStream_t s);
hipError_t sidx_subset_compact(const sidx::u32 *keep, const sidx::u64 *rank, const sidx::i64 *val,
    const sidx::u32 *st, sidx::u64 m, sidx::i64 *cval, sidx::u32 *cst, sidx::u64 *cline, sidx::u64 *ctl,
    hipStream_t s);
hipError_t sidx_subset_init(sidx::u64 *ctl, sidx::u64 nruns, hipStream_t s);
hipError_t sidx_subset_check(const sidx::i64 *cval, const sidx::u32 *cst, sidx::u64 m, sidx::u64 *ctl,
    const sidx::u64 *parent, sidx::u64 parent_count, sidx::i64 ilength, sidx::u64 *rows, sidx::u64 rows_cap,
    sidx::u32 *startf, hipStream_t s);
hipError_t sidx_subset_runs(const sidx::u64 *rows, const sidx::u32 *startf, const sidx::u64 *runid, sidx::u64 m,
    sidx::u64 *ctl, sidx::u64 *runs, sidx::u64 rows_cap, sidx::u64 runs_cap, hipStream_t s);
// the subset walk's slab call (sidx_subset.hip): up to its host stop (the SL_* control words), then
// the closed runs and the carry
hipError_t sidx_subs_plan(const sidx::SubSlabArgs *a, void *scan_tmp, size_t *scan_bytes, hipStream_t s);
hipError_t sidx_subs_commit(const sidx::SubSlabArgs *a, sidx::u64 ke, sidx::u64 nclosed, hipStream_t s);
hipError_t sidx_launch_fq_spans_place(const sidx::SlabParams *pp, sidx::u32 *spans, sidx::u64 *outlen, sidx::u64 K,
    int kind, hipStream_t s);
hipError_t sidx_filter_spans(const uint8_t *data, sidx::u64 n, const sidx::u64 *rows, sidx::u64 K, int kind,
    sidx::u32 *spans, sidx::u64 *outlen, sidx::u64 *firstbad, const sidx::u32 *ord, hipStream_t s);
hipError_t sidx_filter_write(const uint8_t *data, sidx::u64 n, const sidx::u64 *rows, const sidx::u32 *spans,
    const sidx::u64 *outlen, const sidx::u64 *outoff, sidx::u64 K, sidx::u64 total, int kind, sidx::u64 *wfirst,
    uint8_t *out, const sidx::u32 *ord, hipStream_t s);
// the filters' slab step (sidx_filter.hip): spans and writer with the counter *cbase + r + 1, and the
// control kernels around them (st: the FS_* control words, sidx_common.hpp)
hipError_t sidx_filter_spans_base(const uint8_t *data, sidx::u64 n, const sidx::u64 *rows, sidx::u64 K, int kind,
    sidx::u32 *spans, sidx::u64 *outlen, sidx::u64 *firstbad, const sidx::u64 *cbase, hipStream_t s);
hipError_t sidx_filter_write_base(const uint8_t *data, sidx::u64 n, const sidx::u64 *rows, const sidx::u32 *spans,
    const sidx::u64 *outlen, const sidx::u64 *outoff, sidx::u64 K, sidx::u64 total, int kind, sidx::u64 *wfirst,
    uint8_t *out, const sidx::u64 *cbase, hipStream_t s);
hipError_t sidx_filt_slab_begin(const uint8_t *win, sidx::u64 wlo, sidx::u64 whi, sidx::u64 own_end, int first, int last,
    int kind, const sidx::FiltCarry *carry, sidx::u64 *st, hipStream_t s);
hipError_t sidx_filt_slab_settle(const uint8_t *view, sidx::u64 vn, const sidx::u64 *rows, sidx::u64 K, int index_err,
    sidx::u64 own, int last, const sidx::u64 *outlen, const sidx::u64 *outoff, sidx::u64 sec_size, sidx::u64 *st,
    hipStream_t s);
hipError_t sidx_filt_slab_commit(sidx::FiltCarry *carry, const sidx::u64 *st, int first, hipStream_t s);
sidx::u64 sidx_filter_block();
sidx::u32 sidx_filter_recs();
hipError_t sidx_filter_read_status(const uint8_t *data, sidx::u64 n, sidx::u64 start, sidx::u32 *out,
    hipStream_t s);
// the sectioned stream (sidx_stream.hip; control words: sidx_stream.hpp): range check and the sections
// the segmented path leaves to the single-section filter; a batch's records per section; after the
// scan of cnt into base, the batch's rows / ordinals / sections and ctl[SS_KEY], ctl[SS_KE]
hipError_t sidx_stream_classify(const void *d_secs, sidx::u64 nsecs, sidx::u64 n, const int *fmt,
    sidx::u64 small_fastq, sidx::u64 small_fasta, sidx::u64 small_sam, sidx::u64 *ctl, sidx::u64 *others,
    sidx::u64 *cuts, hipStream_t s);
hipError_t sidx_stream_count(const uint8_t *data, sidx::u64 n, const void *d_secs, sidx::u64 S, sidx::u64 *cnt,
    hipStream_t s);
// FASTA / SAM batches: the sections' sequences (boundaries) / lines, the flat rows after the scan, and
// after the spans ctl[SS_KE], ctl[SS_KEY], ctl[SS_NDELIV]
hipError_t sidx_stream_fa_count(const uint8_t *data, sidx::u64 n, const void *d_secs, sidx::u64 S, sidx::u64 *cnt,
    hipStream_t s);
hipError_t sidx_stream_fa_emit(const uint8_t *data, sidx::u64 n, const void *d_secs, sidx::u64 S, const sidx::u64 *cnt,
    const sidx::u64 *base, sidx::u64 *rows, sidx::u32 *ord, sidx::u32 *rsec, hipStream_t s);
hipError_t sidx_stream_sam_count(const uint8_t *data, sidx::u64 n, const void *d_secs, sidx::u64 S, sidx::u64 *cnt,
    hipStream_t s);
hipError_t sidx_stream_sam_emit(const uint8_t *data, sidx::u64 n, const void *d_secs, sidx::u64 S, const sidx::u64 *cnt,
    const sidx::u64 *base, sidx::u64 *rows, sidx::u32 *rsec, hipStream_t s);
hipError_t sidx_stream_flat_finish(const sidx::u32 *rsec, const sidx::u64 *outlen, sidx::u64 K, int count_nz,
    sidx::u64 *ctl, hipStream_t s);
hipError_t sidx_fa_anon_spans_seg(const uint8_t *d, sidx::u64 n, const sidx::u64 *rows, const sidx::u32 *ord,
    sidx::u64 m, sidx::u64 *bspan, sidx::u64 *outlen, sidx::u64 *firstbad, hipStream_t s);
hipError_t sidx_fa_anon_write_seg(const uint8_t *d, sidx::u64 n, const sidx::u64 *bspan, const sidx::u64 *outoff,
    const sidx::u32 *ord, sidx::u64 K, uint8_t *out, hipStream_t s);
hipError_t sidx_stream_index(const uint8_t *data, sidx::u64 n, const void *d_secs, sidx::u64 S, const sidx::u64 *cnt,
    const sidx::u64 *base, sidx::u64 K, sidx::u64 *rows, sidx::u32 *ord, sidx::u32 *rsec, sidx::u64 *ctl,
    hipStream_t s);
// the batch build (sidx_batch.hip; arguments and control words: sidx_batch.hpp): the range check and
// the singles (ctl zeroed by the caller); nat[i] of every node; after the scan of nat into base the
// layout, rows, checks and items (total_bound: row_cap; *launches += the kernels launched)
hipError_t sidx_batch_classify(const sidx::BatchArgs *p, hipStream_t s);
hipError_t sidx_batch_count(const sidx::BatchArgs *p, hipStream_t s);
hipError_t sidx_batch_index(const sidx::BatchArgs *p, sidx::u64 total_bound, sidx::u32 *launches, hipStream_t s);
hipError_t sidx_range_flags(const sidx::u64 *rows, sidx::u64 nrows, sidx::u64 a0, sidx::u64 nr, sidx::u32 *flags,
    hipStream_t s);
hipError_t sidx_range_emit(const sidx::u64 *rows, sidx::u64 nrows, sidx::u64 a0, sidx::u64 nr,
    const sidx::u32 *flags, const sidx::u64 *id, sidx::u64 *recs, hipStream_t s);
hipError_t sidx_gather(const uint8_t *data, sidx::u64 data_len, const sidx::u64 *runs, sidx::u64 bound,
    sidx::u64 *ctl, sidx::u64 *lens, sidx::u64 *outoff, void *tmp, size_t *tmp_bytes, sidx::u64 *wfirst,
    uint8_t *out, sidx::u64 out_cap, hipEvent_t e0, hipEvent_t e1, hipStream_t s);
// the download plan (sidx_plan.hip; control words: sidx_plan.hpp): one level over V > 0 row visits of
// nseg segments (section count into ctl[word], the sections into out when they fit cap); the level-2
// segments of CHUNK_RANGE from the level-1 records; Idx.Part per part
hipError_t sidx_plan_init(sidx::u64 *ctl, hipStream_t s);
hipError_t sidx_plan_level(const sidx::u64 *rows, sidx::u64 nrows, const sidx::u64 *a0, const sidx::u64 *off,
    sidx::u64 nseg, sidx::u64 V, sidx::u32 *flags, sidx::u32 *vseg, sidx::u64 *id, void *tmp, size_t *tmp_bytes,
    sidx::u64 *ctl, int word, sidx::u64 cap, sidx::u64 *out, sidx::u32 *part, const sidx::u32 *segpart,
    sidx::u64 *size, hipStream_t s);
hipError_t sidx_plan_segments(const sidx::u64 *recs, const sidx::u32 *part, sidx::u64 bound, sidx::u64 *ctl,
    sidx::i64 rec_length, sidx::u64 *a0, sidx::u64 *nr, sidx::u64 *off, void *tmp, size_t *tmp_bytes, hipStream_t s);
hipError_t sidx_plan_part(const sidx::u64 *rows, sidx::u64 nrows, const sidx::u64 *a0, const sidx::u64 *b0,
    sidx::u64 P, sidx::u64 *out, sidx::u64 *size, hipStream_t s);

}  // extern "C"
