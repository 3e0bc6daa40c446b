"""GPU: anonymize over whole FASTA and SAM sections past one tile (sidx_filter.hip: k_fa_anon_spans,
k_fa_anon_write, k_sam_anon_spans, k_sam_anon_write; sidx_filter_api.cpp: anonymize_other), byte-exact
against the oracle's filter_fastq(data, "anonymize"), which tests/test_oracle_anonymize.py pins to a
literal transcription of fasta.go / sam.go on every section used here (tests/anonref.py).

Every section goes through filter_device with the output buffer filled with 0xAB and out_cap set to
the exact size: output bytes, count, size, status and error text, and the 64 bytes past the output
still 0xAB (k_fa_anon_write stores whole 16-byte blocks: one it does not own would show there).  Then
once more with out_cap = size - 1: SHOCKIDX_ESPACE, the size reported, nothing written.

The FASTA sections run with both boundary sources: the record index (rows with a stride of 2) and the
unvalidated scan (SHOCKIDX_ANON_SCAN=1; the library reads the variable on every call)."""
import numpy as np
import pytest

import anonref
import kern
from shock_amd import _lib as L
from test_gpu_stream import _check as _stream_check

pytestmark = pytest.mark.gpu
TILE = anonref.TILE
FASTA = dict(anonref.fasta_sections())
SAM = dict(anonref.sam_sections())
_REF = {}


def _ref(oracle, data):
    """The oracle's (out, count, err) of a section, computed once."""
    if data not in _REF:
        _REF[data] = oracle.filter_fastq(data, "anonymize")
    return _REF[data]


def _check(ctx, oracle, data, what=""):
    out, count, err = _ref(oracle, data)
    n, size = len(data), len(out)
    d_in = ctx.alloc(n + 64)
    d_in.upload(data)
    d_out = kern.filled(ctx, size + kern.GUARD, 0xAB)
    try:
        r = ctx.filter_device("anonymize", d_in.ptr, n, d_out.ptr, size)
        assert r.status == (L.OK if err is None else L.EFORMAT), (what, r.status, r.err)
        assert (r.count, r.size, r.err) == (count, size, err), (what, r.count, r.size, r.err, count, size, err)
        got = d_out.download(size + kern.GUARD)
        kern.first_diff(got[:size], np.frombuffer(out, np.uint8), f"{what}: output")
        assert bool((got[size:] == 0xAB).all()), f"{what}: wrote past the output"
        if size:
            d_out.fill(0xAB)
            r = ctx.filter_device("anonymize", d_in.ptr, n, d_out.ptr, size - 1)
            assert r.status == L.ESPACE and r.size == size, (what, r.status, r.size, size)
            assert bool((d_out.download(size + kern.GUARD) == 0xAB).all()), f"{what}: wrote without room"
    finally:
        d_in.free()
        d_out.free()
    return out, count, err


@pytest.fixture(params=["index", "scan"])
def source(request, monkeypatch):
    """The boundary source of a FASTA section."""
    if request.param == "scan":
        monkeypatch.setenv("SHOCKIDX_ANON_SCAN", "1")
    else:
        monkeypatch.delenv("SHOCKIDX_ANON_SCAN", raising=False)
    return request.param


# ---- FASTA ------------------------------------------------------------------------------------------
def test_fasta_grid_stride_gpu(gpu_ctx, oracle_lib, source):
    """270 000 sequences: K > 262144 = 65536 blocks x 4 waves (wave_grid), so the `k += nw` loops of
    k_fa_anon_spans and k_fa_anon_write run a second pass, on the scan path too; the counter's ndigits
    grows at 10, 100, ..., 100 000 (the header width in outlen and in the writer's window)."""
    out, count, err = _check(gpu_ctx, oracle_lib, FASTA["many"], f"many/{source}")
    assert count == 269_999 > 262_144 and err is None


def test_fasta_natural_fallback_gpu(gpu_ctx, oracle_lib, monkeypatch):
    """Headers ending in '>': the record index fails at the first record (build_resident returns
    EFORMAT, `indexed` stays false) and the boundaries come from sidx_fa_bnd_count / _write over 85
    tiles -- without the environment variable.  Read delivers all but the last sequence."""
    monkeypatch.delenv("SHOCKIDX_ANON_SCAN", raising=False)
    data = FASTA["natural-fallback"]
    assert oracle_lib.record_index(data, "fasta")[1] is not None
    assert gpu_ctx.build_host(data, "record", "fasta").status == L.EFORMAT
    out, count, err = _check(gpu_ctx, oracle_lib, data, "natural-fallback")
    assert (count, err) == (100_000, None)


def test_fasta_trims_gpu(gpu_ctx, oracle_lib, source):
    """bytes.TrimSpace at both ends of a read, ASCII and Unicode, at sequence lengths 4..40:
    k_fa_anon_spans' fast path (e0 >= s + 4, `ok(a1)`, `ok(z1)` or an ASCII space before `ok(z2)`)
    next to its bail-outs (a byte >= 0x80 or a space at either end), which run trim_space in lane 0:
    U+0085, U+00A0, U+1680, U+2003, U+2028, U+3000 are trimmed; C2 A1, E2 80 8B, a lone C2 and a cut
    E3 80 are kept."""
    out, count, err = _check(gpu_ctx, oracle_lib, FASTA["trims"], f"trims/{source}")
    assert (count, err) == (anonref.fa_trims()[1], None)


def test_fasta_gt_runs_gpu(gpu_ctx, oracle_lib, source):
    """'>' runs: the lone ">" pieces skipped at a read's start (`while (s < e0 && d[s] == '>')`), the
    TrimRight of the '>'s before the boundary (`while (e > s && d[e - 1] == '>')`), a '>' inside a
    header (no boundary), a body ending in ">\\n" and a lone ">\\n" (Read's error: no '\\n' is left)."""
    for name, data in FASTA.items():
        if name.startswith("gt-runs"):
            _check(gpu_ctx, oracle_lib, data, f"{name}/{source}")


def test_fasta_leading_newlines_gpu(gpu_ctx, oracle_lib, source):
    """The regex skips leading [\\n\\r]*, so the section detects as FASTA; its first read holds nothing
    after the trim: firstbad = 0, Ke = 0, "Invalid fasta entry" with no byte delivered."""
    for name, data in FASTA.items():
        if name.startswith("leading-newlines"):
            assert oracle_lib.detect(data)[0] == "fasta"
            out, count, err = _check(gpu_ctx, oracle_lib, data, f"{name}/{source}")
            assert (out, count, err) == (b"", 0, b"Invalid fasta entry")


def test_fasta_mid_errors_gpu(gpu_ctx, oracle_lib, source):
    """50 000 sequences, the 7th and the 49 998th a header with no body: two waves race on
    atomicMin(firstbad) and the smaller index must win whatever the order (Ke = 6); the scan of the
    lengths and the writer then cover the first six sequences only."""
    out, count, err = _check(gpu_ctx, oracle_lib, FASTA["mid-errors"], f"mid-errors/{source}")
    assert (count, err) == (6, b"Invalid fasta entry") and out.count(b">") == 6
    # 270 000 sequences, the 8th and the 262 148th failing: past wave_grid's cap the later one runs in
    # wave 3 and the earlier in wave 7, so the later error is found by a lower-numbered wave
    out, count, err = _check(gpu_ctx, oracle_lib, FASTA["many-two-errors"], f"many-two-errors/{source}")
    assert (count, err) == (7, b"Invalid fasta entry")


def test_fasta_tile_spanning_gpu(gpu_ctx, oracle_lib, source):
    """A sequence whose '>' sits 1-3 bytes before a tile edge with a body of 0 (Read's error), 1, TILE
    and 2 TILE + 5 bytes in CRLF lines: wave_nl's 1 KiB steps and k_fa_anon_write's 2 KiB steps across
    tiles, the '\\r's kept in the body, the boundary carried into the next tiles on the scan path."""
    for name, data in FASTA.items():
        if name.startswith("tile-spanning"):
            out, count, err = _check(gpu_ctx, oracle_lib, data, f"{name}/{source}")
            assert len(data) < 2 * TILE or (err is None and b"\r" in out)  # the bodies of TILE bytes and more


# ---- SAM --------------------------------------------------------------------------------------------
def test_sam_grid_stride_gpu(gpu_ctx, oracle_lib):
    """270 001 lines, one in ten delivered: K > 262144 puts the `k += nw` loops of k_sam_anon_spans and
    k_sam_anon_write into a second pass; most waves add nothing to the writer's count."""
    data = SAM["many"]
    assert oracle_lib.detect(data)[0] == "sam" and data.count(b"\n") == 270_001
    out, count, err = _check(gpu_ctx, oracle_lib, data, "sam-many")
    assert err is None and 25_000 < count < 29_000


def test_sam_mid_error_gpu(gpu_ctx, oracle_lib):
    """The same with a three-field alignment at line 135 000: `bad < K && bad < eof`, the lines before
    it delivered and counted."""
    data = SAM["many-mid-error"]
    assert oracle_lib.detect(data)[0] == "sam"
    out, count, err = _check(gpu_ctx, oracle_lib, data, "sam-many-mid-error")
    assert err == b"sam alignment fields less than 11" and 10_000 < count < 20_000


def test_sam_field_edges_gpu(gpu_ctx, oracle_lib):
    """`tabs + 1 < 11` over the *trimmed* line: 10 tabs, 9 tabs, 10 tabs of which one leads or trails
    (trimmed away: an error), 11 fields inside tabs, spaces and U+00A0, " @x" (skipped: d[lo] == '@'
    after the trim), lines that are blank after the trim (hi == lo)."""
    for i, (data, fate) in enumerate(anonref.sam_field_edges()):
        assert oracle_lib.detect(data)[0] == "sam"
        out, count, err = _check(gpu_ctx, oracle_lib, data, f"sam-field-edge-{i}")
        assert (count, err is None) == {True: (3, True), None: (2, True), False: (1, False)}[fate]


def test_sam_long_lines_gpu(gpu_ctx, oracle_lib):
    """Lines of 63, 64, 65, 4096, TILE + 3 and 100 000 bytes: the 64-byte steps of the tab count
    (`p += 64`) and of the writer's copy, lines that span tiles of the line index, trim bytes at both
    ends and CRLF endings (the '\\r' goes with the trim)."""
    data = SAM["long-lines"]
    assert oracle_lib.detect(data)[0] == "sam"
    out, count, err = _check(gpu_ctx, oracle_lib, data, "sam-long-lines")
    assert (count, err) == (3 * len(anonref.SAM_LINE_LENGTHS), None) and b"\r" not in out


def test_sam_eof_against_error_gpu(gpu_ctx, oracle_lib):
    """The host's `bad` / `eof` / `Ke`: a bad line before an unterminated last line is the error; the
    unterminated last line as the only bad one is io.EOF (no error); data ending in '\\n' (the line
    index's final (size, 0) row is the EOF); a section that is only its header line."""
    for name, data in anonref.sam_eof_cases():
        assert oracle_lib.detect(data)[0] == "sam"
        _check(gpu_ctx, oracle_lib, data, f"sam-eof-{name}")


# ---- record counts: the size_only route through the sectioned stream ----------------------------------
@pytest.mark.parametrize("which", ["many", "many-mid-error"])
def test_stream_counts_gpu(gpu_ctx, oracle_lib, monkeypatch, which):
    """[small FASTQ, the 270 001-line SAM section, the natural-fallback FASTA section, small FASTQ] in
    one node: the stream sizes every section first (anonymize_other with size_only: the SAM count is the
    number of outlen != 0 among the first Ke lines, the FASTA count Ke), then writes.  With the SAM
    section failing in its middle the stream ends there: err_section == 1 and the bytes before."""
    monkeypatch.delenv("SHOCKIDX_ANON_SCAN", raising=False)
    node, secs = anonref.stream_node(SAM[which])
    assert [oracle_lib.detect(node[p:p + n])[0] for p, n in secs] == ["fastq", "sam", "fasta", "fastq"]
    r = _stream_check(gpu_ctx, oracle_lib, "anonymize", node, secs)
    if which == "many":
        assert r.err_section == -1 and r.count == 2 + _ref(oracle_lib, SAM[which])[1] + 100_000 + 2
    else:
        assert r.err_section == 1 and r.err == b"sam alignment fields less than 11"
        assert r.count == 2 + _ref(oracle_lib, SAM[which])[1]
