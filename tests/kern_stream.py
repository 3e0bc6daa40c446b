"""Direct access to the launchers of the sectioned stream's segmented FASTA and SAM index
(sidx_stream.hip: sidx_stream_fa_count / _fa_emit, sidx_stream_sam_count / _sam_emit, with sidx_scan_u64
between count and emit), in the manner of tests/kern.py: every helper asserts the launcher's
preconditions on the host before it launches, so a mistake in a test fails in Python.

  data   comes from ctx.alloc(n + 64); every section lies inside it and is at most 16 MiB long
  count  cnt holds S words, followed by guard words of 0xAB
  emit   cnt on the device is what count() left and equals the numpy reference (asserted first: a wrong
         count never reaches the emit kernel); base is its exclusive sum; rows hold 2 K words, ord and
         rsec K words each, K = the reference's total, every output followed by guard words of 0xAB
"""
import ctypes

import numpy as np

import anonref
import kern

_vp, _u64, _i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
kern._PROTOS.update({
    # (data, n, secs, S, cnt, stream)
    "sidx_stream_fa_count": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp]),
    "sidx_stream_sam_count": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp]),
    # (data, n, secs, S, cnt, base, rows, ord, rsec, stream)
    "sidx_stream_fa_emit": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    # (data, n, secs, S, cnt, base, rows, rsec, stream)
    "sidx_stream_sam_emit": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
})
SMALL_MAX = 16 << 20  # SS_SMALL_MAX
_AB64, _AB32 = np.uint64(0xABABABABABABABAB), np.uint32(0xABABABAB)


def fasta_ref(data: np.ndarray, secs):
    """-> (cnt[S], rows[K, 2], ord[K], rsec[K]): the flat sequences of the sections, each section's
    boundaries taken over its bytes alone (anonref.fasta_boundaries)."""
    cnt, rows, ords, rsec = [], [], [], []
    for i, (pos, ln) in enumerate(secs):
        b = anonref.fasta_boundaries(data[pos:pos + ln]).astype(np.int64) + pos
        cnt.append(len(b))
        starts = np.concatenate([[pos], b[:-1]]) if len(b) else b
        rows.append(np.stack([starts, b], axis=1).reshape(-1, 2))
        ords.append(np.arange(len(b)))
        rsec.append(np.full(len(b), i))
    return (np.array(cnt, np.uint64), np.concatenate(rows).astype(np.uint64).reshape(-1, 2),
            np.concatenate(ords).astype(np.uint32), np.concatenate(rsec).astype(np.uint32))


def sam_ref(data: np.ndarray, secs):
    """-> (cnt[S], rows[K, 2], rsec[K]): the '\\n'-terminated lines (offset, length) of the sections."""
    cnt, rows, rsec = [], [], []
    for i, (pos, ln) in enumerate(secs):
        e = np.flatnonzero(data[pos:pos + ln] == 10).astype(np.int64) + pos + 1
        cnt.append(len(e))
        starts = np.concatenate([[pos], e[:-1]]) if len(e) else e
        rows.append(np.stack([starts, e - starts], axis=1).reshape(-1, 2))
        rsec.append(np.full(len(e), i))
    return (np.array(cnt, np.uint64), np.concatenate(rows).astype(np.uint64).reshape(-1, 2),
            np.concatenate(rsec).astype(np.uint32))


class IndexJob:
    """One section list through count, scan and emit of one format ("fasta" or "sam")."""

    def __init__(self, ctx, fmt: str, data, secs):
        assert fmt in ("fasta", "sam")
        a = np.ascontiguousarray(data)
        assert a.dtype == np.uint8 and a.ndim == 1
        secs = np.ascontiguousarray(secs, dtype=np.int64).reshape(-1, 2)
        assert len(secs) >= 1
        for pos, ln in secs.tolist():
            assert 0 <= pos and 0 <= ln <= SMALL_MAX and pos + ln <= len(a), (pos, ln, len(a))
        self.ctx, self.fmt, self.n, self.S, self.secs = ctx, fmt, len(a), len(secs), secs
        self.d_data = kern.upload(ctx, a, 64)
        self.d_secs = kern.upload(ctx, secs, 64)
        self.d_cnt = kern.filled(ctx, 8 * (self.S + kern.GUARD), 0xAB)
        self.d_base = kern.filled(ctx, 8 * (self.S + kern.GUARD), 0xAB)
        self.bufs = [self.d_data, self.d_secs, self.d_cnt, self.d_base]
        self.counted = None

    def count(self):
        """-> cnt with its guard words"""
        assert self.d_data.nbytes >= self.n + 64 and self.d_cnt.nbytes >= 8 * self.S and self.d_secs.nbytes >= 16 * self.S
        rc = kern.fn(f"sidx_stream_{'fa' if self.fmt == 'fasta' else 'sam'}_count")(
            self.d_data.ptr, self.n, self.d_secs.ptr, self.S, self.d_cnt.ptr, self.ctx.stream)
        assert rc == kern.HIP_SUCCESS, rc
        self.ctx.sync()
        got = kern.download(self.d_cnt, np.uint64, self.S + kern.GUARD)
        self.counted = got[:self.S].copy()
        return got

    def emit(self, cnt_ref):
        """-> (base, rows, ord | None, rsec), each with its guard words; cnt_ref: the reference count."""
        assert self.counted is not None and np.array_equal(self.counted, cnt_ref), "count() first, and it must be right"
        K = int(cnt_ref.sum())
        need = kern.scan_tmp_bytes(self.ctx, "u64", self.S)
        d_tmp = self.ctx.alloc(need)
        d_rows = kern.filled(self.ctx, 8 * (2 * K + kern.GUARD), 0xAB)
        d_ord = kern.filled(self.ctx, 4 * (K + kern.GUARD), 0xAB)
        d_rsec = kern.filled(self.ctx, 4 * (K + kern.GUARD), 0xAB)
        self.bufs += [d_tmp, d_rows, d_ord, d_rsec]
        sb = ctypes.c_size_t(need)
        assert d_tmp.nbytes >= need and d_tmp.ptr % 16 == 0 and self.d_base.nbytes >= 8 * self.S
        rc = kern.fn("sidx_scan_u64")(self.d_cnt.ptr, self.d_base.ptr, self.S, d_tmp.ptr, ctypes.byref(sb), self.ctx.stream)
        assert rc == kern.HIP_SUCCESS, rc
        assert d_rows.nbytes >= 16 * K and d_ord.nbytes >= 4 * K and d_rsec.nbytes >= 4 * K
        if self.fmt == "fasta":
            rc = kern.fn("sidx_stream_fa_emit")(self.d_data.ptr, self.n, self.d_secs.ptr, self.S, self.d_cnt.ptr,
                                                self.d_base.ptr, d_rows.ptr, d_ord.ptr, d_rsec.ptr, self.ctx.stream)
        else:
            rc = kern.fn("sidx_stream_sam_emit")(self.d_data.ptr, self.n, self.d_secs.ptr, self.S, self.d_cnt.ptr,
                                                 self.d_base.ptr, d_rows.ptr, d_rsec.ptr, self.ctx.stream)
        assert rc == kern.HIP_SUCCESS, rc
        self.ctx.sync()
        return (kern.download(self.d_base, np.uint64, self.S + kern.GUARD), kern.download(d_rows, np.uint64, 2 * K + kern.GUARD),
                kern.download(d_ord, np.uint32, K + kern.GUARD), kern.download(d_rsec, np.uint32, K + kern.GUARD))

    def check(self, what=""):
        """count, scan and emit against the numpy reference, guard words included."""
        data = self.d_data.download(self.n)
        secs = self.secs.tolist()
        if self.fmt == "fasta":
            cnt, rows, ords, rsec = fasta_ref(data, secs)
        else:
            cnt, rows, rsec = sam_ref(data, secs)
            ords = None
        got = self.count()
        kern.first_diff(got[:self.S], cnt, f"{what}: cnt")
        assert bool((got[self.S:] == _AB64).all()), f"{what}: cnt wrote past the output"
        K = int(cnt.sum())
        base, grows, gord, grsec = self.emit(cnt)
        kern.first_diff(base[:self.S], kern.scan_ref("u64", cnt), f"{what}: base")
        kern.first_diff(grows[:2 * K], rows.reshape(-1), f"{what}: rows")
        kern.first_diff(grsec[:K], rsec, f"{what}: rsec")
        assert bool((base[self.S:] == _AB64).all()) and bool((grows[2 * K:] == _AB64).all()), f"{what}: wrote past rows"
        assert bool((grsec[K:] == _AB32).all()), f"{what}: wrote past rsec"
        if ords is not None:
            kern.first_diff(gord[:K], ords, f"{what}: ord")
            assert bool((gord[K:] == _AB32).all()), f"{what}: wrote past ord"
        else:
            assert bool((gord == _AB32).all()), f"{what}: SAM emit wrote ordinals"
        return K

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []
