"""Direct access to the launchers behind the public entry points, for tests that need counts or
counters no input file of test size produces: the device-wide scans (sidx_scan.hpp through
sidx_scan_flags / sidx_scan_u64 / sidx_scan_max_u64 / sidx_crs_scan), the FASTQ filter writer
(sidx_filter.hip through sidx_filter_spans / sidx_filter_write) and the FASTA boundary scan of anonymize
(sidx_filter.hip through sidx_fa_bnd_count / sidx_fa_bnd_write).  Every launcher returns hipError_t
as an int (0: success).  All launches go to ctx.stream; buffers come from ctx.alloc.

A launcher trusts its caller, so every helper here asserts the launcher's preconditions on the host
before it launches -- a mistake in a test fails in Python and never reaches the device:

  scans    the input holds n items, the output n words (sidx_crs_scan: R rows in, R words of lengths
           and R + 1 words of sums out); the workspace buffer holds at least the queried size (the
           size *claimed* to the launcher may be smaller: it then refuses without launching);
           running totals stay below 2^62 (the look-back words' payload)
  spans    data comes from ctx.alloc(len + 64); every row is a whole four-line record inside data
           that starts with '@' and ends in '\\n'; ord (when given) holds one u32 per row; outlen is
           zeroed before the launch (bit 63 means "already placed"); firstbad starts as ~0
  write    spans() ran and every span lies inside its record; outoff is the exact exclusive sum of
           the downloaded outlen; wfirst has total / block + 4 words; out has total + 64 bytes, is
           16-byte aligned and is filled with 0xAB before the launch
  fa bnd   data comes from ctx.alloc(n + 64), n >= 1; with nt = ceil(n / TILE) tiles, lnl / lgt / cnl / cgt /
           tcnt / toff hold nt + 1 words each and slot sidx_fa_slot() * (nt + 1) u16s; tmp holds the queried
           size; for the write, tcnt / toff are what the count left (checked against the reference first: a
           wrong count never reaches the writer) and B holds K = toff[nt-1] + tcnt[nt-1] words, K at most
           the number of '>' in data, followed by guard words of 0xAB
"""
import ctypes

import numpy as np

from shock_amd import _lib as L

HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1
FQ2FA, ANON = 1, 2  # FilterKind (sidx_filter.hip)
KINDS = {"fq2fa": FQ2FA, "anonymize": ANON}
GUARD = 64  # words (scans) / bytes (writer) past the output that must stay 0xAB
PAY_MAX = (1 << 62) - 1  # the largest running total a scan may reach

_vp, _u64, _i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
_psz = ctypes.POINTER(ctypes.c_size_t)
_PROTOS = {
    "sidx_scan_block": (_u64, []),
    "sidx_scan_small_items": (_u64, []),
    "sidx_filter_block": (_u64, []),
    "sidx_filter_recs": (ctypes.c_uint32, []),
    "sidx_fa_slot": (ctypes.c_uint32, []),
    # (data, n, lnl, lgt, cnl, cgt, tcnt, toff, slot, tmp, tmp_bytes, stream)
    "sidx_fa_bnd_count": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _psz, _vp]),
    # (data, n, cnl, cgt, tcnt, toff, slot, B, stream)
    "sidx_fa_bnd_write": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # (in, out, n, tmp, tmp_bytes, stream)
    "sidx_scan_flags": (_i32, [_vp, _vp, _u64, _vp, _psz, _vp]),
    "sidx_scan_u64": (_i32, [_vp, _vp, _u64, _vp, _psz, _vp]),
    "sidx_scan_max_u64": (_i32, [_vp, _vp, _u64, _vp, _psz, _vp]),
    # (ri, R, len, P, tmp, scan_bytes, stream)
    "sidx_crs_scan": (_i32, [_vp, _u64, _vp, _vp, _vp, _psz, _vp]),
    # (data, n, rows, K, kind, spans, outlen, firstbad, ord, stream)
    "sidx_filter_spans": (_i32, [_vp, _u64, _vp, _u64, _i32, _vp, _vp, _vp, _vp, _vp]),
    # (data, n, rows, spans, outlen, outoff, K, total, kind, wfirst, out, ord, stream)
    "sidx_filter_write": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _i32, _vp, _vp, _vp, _vp]),
}
_bound = {}


def fn(name):
    if name not in _bound:
        f = getattr(L.lib(), name)
        f.restype, f.argtypes = _PROTOS[name]
        _bound[name] = f
    return _bound[name]


def scan_block() -> int:
    return int(fn("sidx_scan_block")())


def scan_small_items() -> int:
    return int(fn("sidx_scan_small_items")())


def filter_block() -> int:
    return int(fn("sidx_filter_block")())


def filter_recs() -> int:
    return int(fn("sidx_filter_recs")())


# ---- buffers --------------------------------------------------------------------------------------
def upload(ctx, arr, extra: int = 0):
    """A device buffer holding arr's bytes (+ extra bytes of room); the copy is waited for."""
    a = np.ascontiguousarray(arr)
    buf = ctx.alloc(a.nbytes + extra)
    buf.upload(a.view(np.uint8).reshape(-1))
    return buf


def download(buf, dtype, count: int, offset: int = 0):
    dt = np.dtype(dtype)
    assert offset + count * dt.itemsize <= buf.nbytes
    return buf.download(count * dt.itemsize, offset).view(dt)


def filled(ctx, nbytes: int, value: int):
    buf = ctx.alloc(nbytes)
    buf.fill(value)
    return buf


def first_diff(got, exp, what=""):
    """Whole-array equality; a mismatch names the first differing index and both values."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        i = int(np.flatnonzero(got != exp)[0])
        raise AssertionError(f"{what}: first difference at index {i} of {len(exp)}: got {int(got[i])}, "
                             f"expected {int(exp[i])} ({int((got != exp).sum())} differ)")


# ---- scans ------------------------------------------------------------------------------------------
SCANS = ("flags", "u64", "max", "crs")
_SCAN_FN = {"flags": "sidx_scan_flags", "u64": "sidx_scan_u64", "max": "sidx_scan_max_u64", "crs": "sidx_crs_scan"}
_AB64 = np.uint64(0xABABABABABABABAB)


def scan_tmp_bytes(ctx, which: str, n: int) -> int:
    """The size query (tmp == NULL)."""
    sb = ctypes.c_size_t(0)
    if which == "crs":
        rc = fn("sidx_crs_scan")(None, n, None, None, None, ctypes.byref(sb), ctx.stream)
    else:
        rc = fn(_SCAN_FN[which])(None, None, n, None, ctypes.byref(sb), ctx.stream)
    assert rc == HIP_SUCCESS and sb.value >= 16, (which, n, rc, sb.value)
    return int(sb.value)


def scan_ref(which: str, values):
    """The exact result in uint64: flags / u64: exclusive sums; max: exclusive running maximum (the
    identity is 0); crs: values are (offset, length) rows, the result P[0] = 0, P[i + 1] = the
    inclusive sum of the lengths (k_crs_len takes a row's second word as its length)."""
    v = np.asarray(values)
    w = (v.reshape(-1, 2)[:, 1] if which == "crs" else v).astype(np.uint64)
    assert len(w) == 0 or int(w.max()) <= PAY_MAX
    out = np.zeros(len(w), np.uint64)
    if which == "max":
        if len(w) > 1:
            out[1:] = np.maximum.accumulate(w)[:-1]
        return out
    inc = np.cumsum(w, dtype=np.uint64)
    # no wrap-around: the inclusive sums of non-negative items never decrease
    assert len(w) == 0 or (int(inc[-1]) <= PAY_MAX and bool((inc[1:] >= inc[:-1]).all())), which
    if which == "crs":
        return np.concatenate([out[:1] if len(w) else np.zeros(1, np.uint64), inc])
    out[1:] = inc[:-1]
    return out


class ScanJob:
    """One scan's device buffers: the input, and the output followed by GUARD words of 0xAB.
    launch() only enqueues on ctx.stream (several jobs may share one workspace back to back);
    result() waits and downloads the output with its guard words."""

    def __init__(self, ctx, which: str, values):
        assert which in SCANS
        self.ctx, self.which = ctx, which
        v = np.ascontiguousarray(values)
        if which == "flags":
            assert v.dtype == np.uint32 and v.ndim == 1
            self.n, self.nout = len(v), len(v)
        elif which == "crs":
            assert v.dtype == np.uint64 and v.ndim == 2 and v.shape[1] == 2
            self.n, self.nout = len(v), len(v) + 1
        else:
            assert v.dtype == np.uint64 and v.ndim == 1
            self.n, self.nout = len(v), len(v)
        self.exp = scan_ref(which, v)  # also checks the 2^62 limit
        assert len(self.exp) == self.nout
        self.d_in = upload(ctx, v, 64)
        self.d_out = filled(ctx, 8 * (self.nout + GUARD), 0xAB)
        self.d_len = filled(ctx, 8 * (self.n + GUARD), 0xAB) if which == "crs" else None
        self.need = scan_tmp_bytes(ctx, which, self.n) if self.n else scan_tmp_bytes(ctx, which, 1)

    def launch(self, tmp, claim: int | None = None) -> int:
        """tmp: the workspace buffer, at least the queried size; claim: the size told to the launcher."""
        assert tmp.nbytes >= self.need and tmp.ptr and tmp.ptr % 16 == 0
        assert self.d_in.nbytes >= self.n * (4 if self.which == "flags" else 16 if self.which == "crs" else 8)
        assert self.d_out.nbytes >= 8 * self.nout
        sb = ctypes.c_size_t(self.need if claim is None else claim)
        assert sb.value <= tmp.nbytes
        if self.which == "crs":
            assert self.d_len.nbytes >= 8 * self.n
            return fn("sidx_crs_scan")(self.d_in.ptr, self.n, self.d_len.ptr, self.d_out.ptr, tmp.ptr, ctypes.byref(sb),
                                       self.ctx.stream)
        return fn(_SCAN_FN[self.which])(self.d_in.ptr, self.d_out.ptr, self.n, tmp.ptr, ctypes.byref(sb), self.ctx.stream)

    def result(self):
        self.ctx.sync()
        return download(self.d_out, np.uint64, self.nout + GUARD)

    def lengths(self):
        """sidx_crs_scan's second output (the rows' lengths) with its guard words."""
        self.ctx.sync()
        return download(self.d_len, np.uint64, self.n + GUARD)

    def check(self, got=None, what=""):
        got = self.result() if got is None else got
        first_diff(got[:self.nout], self.exp, f"{self.which} n={self.n} {what}")
        assert bool((got[self.nout:] == _AB64).all()), f"{self.which} n={self.n} {what}: wrote past the output"

    def free(self):
        for b in (self.d_in, self.d_out, self.d_len):
            if b is not None:
                b.free()


# ---- the FASTQ filter writer -----------------------------------------------------------------------
_REC_REF = {}
DETECT_WINDOW = 32768  # bytes of a section that the format detection reads (anonymize detects first)
CARRIER = b"@a\nA\n+\nI\n"


def record_ref(oracle, name: str, rec: bytes, counter: int) -> bytes:
    """The reference output of one record of a row table: the oracle's output of the record delivered
    alone, under anonymize with its leading "@1\n" replaced by "@<counter>\n".  A record the oracle does
    not deliver alone (count != 1 or an error, e.g. one that fails the standalone format detection) is
    not allowed here.  The one exception is a record of DETECT_WINDOW bytes and more, which no detection
    can see whole: it is delivered as the second record behind the minimal CARRIER, and the carrier's
    output is taken off.  tests/test_writer_ref.py proves both compositions against whole sections."""
    key = (name, rec)
    if key not in _REC_REF:
        if len(rec) >= DETECT_WINDOW:
            head = record_ref(oracle, name, CARRIER, 1)
            out, count, err = oracle.filter_fastq(CARRIER + rec, name)
            assert count == 2 and err is None and out.startswith(head), (name, rec[:60], count, err)
            out = out[len(head):]
            assert name != "anonymize" or out.startswith(b"@2\n")
            out = (b"@1\n" + out[3:]) if name == "anonymize" else out
        else:
            out, count, err = oracle.filter_fastq(rec, name)
            assert count == 1 and err is None, (name, rec[:60], count, err)
            assert name != "anonymize" or out.startswith(b"@1\n")
        _REC_REF[key] = out
    out = _REC_REF[key]
    return b"@%d\n" % counter + out[3:] if name == "anonymize" else out


def section_ref(oracle, name: str, recs, counters=None):
    """-> [each record's reference output], in row order; counters default to 1, 2, ..."""
    return [record_ref(oracle, name, r, counters[i] if counters is not None else i + 1) for i, r in enumerate(recs)]


class WriterCase:
    """One section through sidx_filter_spans and sidx_filter_write with a caller-made row table and
    (for anonymize) caller-made ordinals: record r's counter is ord[r] + 1, or r + 1 without ord."""

    def __init__(self, ctx, data: bytes, rows, kind: int, ord=None):
        assert kind in (FQ2FA, ANON)
        self.ctx, self.kind, self.n = ctx, kind, len(data)
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
        self.K = len(rows)
        assert self.K >= 1
        for off, ln in rows.tolist():  # whole four-line records inside data
            rec = data[off:off + ln]
            assert off + ln <= len(data) and ln >= 8 and ln < 1 << 31, (off, ln)
            assert rec[:1] == b"@" and rec[-1:] == b"\n" and rec.count(b"\n") == 4, (off, rec[:40])
        self.rows = rows
        if ord is not None:
            assert kind == ANON
            ord = np.ascontiguousarray(ord, dtype=np.uint64)
            assert len(ord) == self.K and int(ord.max()) < 1 << 32
            ord = ord.astype(np.uint32)
        self.ord = ord
        self.d_data = ctx.alloc(len(data) + 64)  # the launchers' loads may run 64 bytes past the section
        self.d_data.upload(data)
        self.d_rows = upload(ctx, rows)
        self.d_ord = upload(ctx, ord) if ord is not None else None
        self.d_spans = ctx.alloc(24 * self.K + 64)
        self.d_outlen = ctx.alloc(8 * self.K + 64)
        self.d_small = ctx.alloc(64)
        self.bufs = [self.d_data, self.d_rows, self.d_spans, self.d_outlen, self.d_small] + ([self.d_ord] if ord is not None else [])
        self.outlen = None

    def spans(self):
        """k_fq_spans -> (outlen[K], firstbad)."""
        self.d_outlen.fill(0)  # bit 63 of a word would mean "already placed"
        self.d_small.fill(0xFF)  # firstbad = ~0
        assert self.d_data.nbytes >= self.n + 64 and self.d_spans.nbytes >= 24 * self.K
        rc = fn("sidx_filter_spans")(self.d_data.ptr, self.n, self.d_rows.ptr, self.K, self.kind, self.d_spans.ptr,
                                     self.d_outlen.ptr, self.d_small.ptr, self.d_ord.ptr if self.d_ord else None,
                                     self.ctx.stream)
        assert rc == HIP_SUCCESS, rc
        self.ctx.sync()
        self.outlen = download(self.d_outlen, np.uint64, self.K)
        self.sp = download(self.d_spans, np.uint32, 6 * self.K).reshape(-1, 6).astype(np.uint64)
        return self.outlen, int(download(self.d_small, np.uint64, 1)[0])

    def write(self, outoff):
        """k_fw_plan + k_fq_write -> the output with GUARD bytes past it, and wfirst's first nblocks words."""
        assert self.outlen is not None, "spans() first"
        ln = self.rows[:, 1]
        for a, b in ((0, 1), (2, 3), (4, 5)):  # every span inside its record
            assert bool((self.sp[:, a] + self.sp[:, b] <= ln).all())
        assert bool((self.outlen > 0).all()) and int(self.outlen.max()) < 1 << 40
        outoff = np.ascontiguousarray(outoff, dtype=np.uint64)
        exact = np.concatenate([np.zeros(1, np.uint64), np.cumsum(self.outlen, dtype=np.uint64)])
        assert np.array_equal(outoff, exact[:-1]), "outoff is not the exclusive sum of outlen"
        total, block = int(exact[-1]), filter_block()
        d_off = upload(self.ctx, outoff, 64)
        nwf = total // block + 4
        d_wf = filled(self.ctx, 8 * nwf, 0xFF)
        d_out = filled(self.ctx, total + GUARD, 0xAB)
        self.bufs += [d_off, d_wf, d_out]
        assert d_out.ptr % 16 == 0 and d_out.nbytes >= total and d_wf.nbytes >= 8 * (total // block + 4)
        rc = fn("sidx_filter_write")(self.d_data.ptr, self.n, self.d_rows.ptr, self.d_spans.ptr, self.d_outlen.ptr,
                                     d_off.ptr, self.K, total, self.kind, d_wf.ptr, d_out.ptr,
                                     self.d_ord.ptr if self.d_ord else None, self.ctx.stream)
        assert rc == HIP_SUCCESS, rc
        self.ctx.sync()
        nblocks = (total + block - 1) // block
        return d_out.download(total + GUARD).tobytes(), download(d_wf, np.uint64, nblocks)

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


# ---- the FASTA boundary scan (anonymize over a section whose record index fails) --------------------
TILE = 16384  # SIDX_TILE


def fa_slot() -> int:
    return int(fn("sidx_fa_slot")())


class FaBoundaryJob:
    """One buffer through sidx_fa_bnd_count (k_fa_last, the two max scans, k_fa_bnd, the sum scan) and
    sidx_fa_bnd_write (k_fa_bwrite).  count() -> (tcnt[nt], toff[nt], slot[nt, FSLOT]); write(K) -> B with
    its guard words.  The guard is a whole tile of words: every '>' of a last tile, were they all
    written past the end, still lands inside the allocation."""
    BGUARD = TILE

    def __init__(self, ctx, data):
        a = np.ascontiguousarray(data)
        assert a.dtype == np.uint8 and a.ndim == 1 and len(a) >= 1
        self.ctx, self.n, self.nt = ctx, len(a), (len(a) + TILE - 1) // TILE
        self.ngt = int((a == 0x3E).sum())
        self.d_data = upload(ctx, a, 64)  # the loads may run 64 bytes past the buffer
        w = self.nt + 1
        self.words = [filled(ctx, 8 * w, 0xAB) for _ in range(6)]  # lnl lgt cnl cgt tcnt toff
        self.d_slot = filled(ctx, 2 * fa_slot() * w, 0xAB)
        sb = ctypes.c_size_t(0)
        rc = fn("sidx_fa_bnd_count")(None, self.n, None, None, None, None, None, None, None, None, ctypes.byref(sb), ctx.stream)
        assert rc == HIP_SUCCESS and sb.value >= 16, (rc, sb.value)
        self.need = int(sb.value)
        self.d_tmp = ctx.alloc(self.need)
        self.bufs = [self.d_data, self.d_slot, self.d_tmp] + self.words
        self.K = None

    def count(self):
        w = self.nt + 1
        assert self.d_data.nbytes >= self.n + 64 and all(b.nbytes >= 8 * w for b in self.words)
        assert self.d_slot.nbytes >= 2 * fa_slot() * w and self.d_tmp.nbytes >= self.need and self.d_tmp.ptr % 16 == 0
        sb = ctypes.c_size_t(self.need)
        rc = fn("sidx_fa_bnd_count")(self.d_data.ptr, self.n, *[b.ptr for b in self.words], self.d_slot.ptr, self.d_tmp.ptr,
                                     ctypes.byref(sb), self.ctx.stream)
        assert rc == HIP_SUCCESS, rc
        self.ctx.sync()
        tcnt, toff = download(self.words[4], np.uint64, self.nt), download(self.words[5], np.uint64, self.nt)
        slot = download(self.d_slot, np.uint16, fa_slot() * self.nt).reshape(self.nt, fa_slot())
        return tcnt, toff, slot

    def write(self, K: int):
        """K: toff[nt-1] + tcnt[nt-1] of a count() the caller has compared with the reference."""
        assert 0 <= K <= self.ngt, (K, self.ngt)
        self.K = K
        d_B = filled(self.ctx, 8 * (K + self.BGUARD), 0xAB)
        self.bufs.append(d_B)
        assert d_B.nbytes >= 8 * (K + self.BGUARD)
        rc = fn("sidx_fa_bnd_write")(self.d_data.ptr, self.n, self.words[2].ptr, self.words[3].ptr, self.words[4].ptr,
                                     self.words[5].ptr, self.d_slot.ptr, d_B.ptr, self.ctx.stream)
        assert rc == HIP_SUCCESS, rc
        self.ctx.sync()
        return download(d_B, np.uint64, K + self.BGUARD)

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []
