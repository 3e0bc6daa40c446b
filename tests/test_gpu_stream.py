"""GPU: the sectioned stream (request/streamer.go:78-98 with a Filter) in one device call,
shockidx_stream_filter_device.  Every case is compared byte-exact with the composition rule over the
oracle's single-section filter (tests/streamref.py) and with a loop of filter_host over the sections
(what the library offered before): output, record count, byte count, status, error text and the failing
section."""
import ctypes
import os
import random

import numpy as np
import pytest

import gen
import streamref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "fixtures")
NAMES = ("fq2fa", "anonymize")
KATS = streamref.load_kats()


def _loop(ctx, name, data, secs):
    """The per-section loop of the single-section entry point, composed like the Streamer composes."""
    out, count = [], 0
    for i, (pos, ln) in enumerate(secs):
        r = ctx.filter_host(name, data[pos:pos + ln])
        assert r.status in (0, 1), (r.status, r.err)
        out.append(r.gathered)
        count += r.count
        if r.status == 1:
            return b"".join(out), count, r.err, i
    return b"".join(out), count, None, -1


def _check(ctx, oracle, name, data, secs):
    secs = [(int(p), int(n)) for p, n in secs]
    exp = streamref.stream_ref(oracle, name, data, secs)
    assert _loop(ctx, name, data, secs) == exp
    r = ctx.stream_filter_host(name, data, secs)
    assert r.status in (0, 1), (r.status, r.err)
    got = (r.gathered, r.count, r.err, r.err_section)
    assert got == exp, (name, secs[:8], got[1:], exp[1:])
    assert r.size == len(exp[0]) and r.status == (0 if exp[2] is None else 1)
    return r


def _records(ctx, data):
    """The record index's rows of a well-formed FASTQ buffer as [(pos, len)]."""
    r = ctx.build_host(data, "record", "fastq")
    assert r.ok
    return [(int(o), int(n)) for o, n in r.rows]


def _cut(rng, rows, lo, hi):
    """Consecutive sections of lo..hi records each."""
    secs, i = [], 0
    while i < len(rows):
        k = min(len(rows) - i, rng.randint(lo, hi))
        secs.append((rows[i][0], rows[i + k - 1][0] + rows[i + k - 1][1] - rows[i][0]))
        i += k
    return secs


@pytest.fixture(scope="module")
def sample():
    return open(os.path.join(FIX, "sample1.fq"), "rb").read()


@pytest.mark.parametrize("kat", KATS, ids=[k[0] for k in KATS])
def test_stream_kats_gpu(gpu_ctx, oracle_lib, kat):
    _, name, data, secs, out, esec, err = kat
    r = _check(gpu_ctx, oracle_lib, name, data, secs)
    assert (r.gathered, r.err, r.err_section) == (out, err, esec)


def test_stream_sample_sections_gpu(gpu_ctx, oracle_lib, sample):
    """sample1.fq (25 records): one-record sections, the runs of a subset, reversed, one listed twice."""
    rows = _records(gpu_ctx, sample)
    assert len(rows) == 25
    sub = gpu_ctx.subset_host(b"1\n2\n3\n7\n8\n20\n", np.array(rows, dtype=np.uint64))
    runs = [(int(o), int(n)) for o, n in sub.run_rows]
    assert len(runs) == 3
    for name in NAMES:
        _check(gpu_ctx, oracle_lib, name, sample, rows)
        _check(gpu_ctx, oracle_lib, name, sample, runs)
        _check(gpu_ctx, oracle_lib, name, sample, rows[::-1])
        _check(gpu_ctx, oracle_lib, name, sample, runs + [runs[1]] + rows[3:6] + [rows[4]])


def test_stream_counter_width_gpu(gpu_ctx, oracle_lib, sample):
    """Two sections of 12 records under anonymize: @9, @10, ... and then @1 again."""
    rows = _records(gpu_ctx, sample)
    secs = [(rows[0][0], rows[12][0] - rows[0][0]), (rows[12][0], rows[24][0] - rows[12][0])]
    r = _check(gpu_ctx, oracle_lib, "anonymize", sample, secs)
    ids = [ln for ln in r.gathered.split(b"\n")[0::4] if ln]
    assert ids == [b"@%d" % (k + 1) for k in range(12)] * 2


def test_stream_unaligned_cuts_gpu(gpu_ctx, oracle_lib, sample):
    """Cuts that are not record-aligned; some end in a reader error, which is the expected result."""
    rows = _records(gpu_ctx, sample)
    blank = sample[:rows[5][0]] + b"\n" + sample[rows[5][0]:]  # a blank line before record 5
    b5 = rows[5][0]
    q3 = rows[3][0] + rows[3][1] - 4  # inside record 3's quality line
    end = len(sample)
    cases = [
        (blank, [(0, b5), (b5, 200), (0, b5)]),              # a section starting on a blank line
        (blank, [(0, b5 + 1), (b5 + 1, len(blank) - b5 - 1)]),  # a section ending on "\n\n"
        (sample, [(rows[2][0] + 5, 300), (0, 100)]),         # a section starting mid-record
        (sample, [(0, q3), (rows[4][0], end - rows[4][0])]),  # ending mid-quality-line, mid-list: dropped
        (sample, [(0, rows[3][0] + 9), (rows[4][0], 50)]),   # ending inside an ID line: truncated
        (sample, [(rows[1][0], rows[6][0] - rows[1][0] - 1), (rows[6][0], end - rows[6][0])]),  # last '\n' cut off
    ]
    for data, secs in cases:
        for name in NAMES:
            _check(gpu_ctx, oracle_lib, name, data, secs)


@pytest.mark.parametrize("seed", range(16))
def test_stream_random_gpu(gpu_ctx, oracle_lib, seed):
    """gen.fastq with CRLF and Unicode space, half of them corrupted, cut at seeded record boundaries
    into 1-40-record sections: the error section and the bytes before the error."""
    rng = random.Random(500 + seed)
    good = gen.fastq(rng, rng.randint(200, 400), crlf=0.3 if seed % 3 == 0 else 0.0, plus_id=0.3,
                     uni=0.1 if seed % 4 == 2 else 0.0)
    rows = _records(gpu_ctx, good)
    data = good
    if seed % 2:
        kind = gen.FASTQ_CORRUPTIONS[(seed // 2) % len(gen.FASTQ_CORRUPTIONS)]
        data = gen.fastq_corrupt(rng, good, kind)
    secs = [(p, min(n, max(0, len(data) - p))) for p, n in _cut(rng, rows, 1, 40) if p <= len(data)]
    for name in NAMES:
        r = _check(gpu_ctx, oracle_lib, name, data, secs)
        if r.err is not None:
            assert 0 <= r.err_section < len(secs)


def test_stream_alignment_gpu(gpu_ctx, oracle_lib):
    """data_len not a multiple of 16 with the last section ending at data_len; sections starting at
    offsets 1-15 past a 16-byte line."""
    rec = b"@r123456\nACGTACGTACGTACG\n+\nIIIIIIIIIIIIIII\n"  # 9 + 16 + 2 + 16 = 43 bytes
    for lead in range(1, 16):
        data = b"x" * 15 + b"\n" + b"y" * (lead - 1) + b"\n" + rec * 3 + rec[:-1]
        assert len(data) % 16 != 0 or lead == 5
        s0 = 16 + lead
        secs = [(s0, 43), (s0 + 43, 86), (s0 + 129, len(data) - s0 - 129), (s0 + 86, len(data) - s0 - 86)]
        for name in NAMES:
            _check(gpu_ctx, oracle_lib, name, data, secs)
    data = rec * 5 + b"@t\nA\n+\nI"  # 223 bytes
    assert len(data) % 16
    _check(gpu_ctx, oracle_lib, "fq2fa", data, [(43, 43), (86, len(data) - 86)])


def test_stream_writer_seams_gpu(gpu_ctx, oracle_lib):
    """A total output of at least 5 writer blocks, with section boundaries inside blocks."""
    from shock_amd import _lib as L
    fn = L.lib().sidx_filter_block
    fn.restype = ctypes.c_uint64
    block = int(fn())
    rng = random.Random(9)
    data = gen.fastq(rng, 1400, plus_id=0.2)
    rows = _records(gpu_ctx, data)
    secs = _cut(rng, rows, 1, 30)
    for name in NAMES:
        r = _check(gpu_ctx, oracle_lib, name, data, secs)
        assert r.size >= 5 * block
    # where the sections' outputs start: not on block boundaries
    offs = np.cumsum([len(oracle_lib.filter_fastq(data[p:p + n], "fq2fa")[0]) for p, n in secs])
    assert sum(1 for o in offs if o % block) >= len(secs) - 5


def _mixed_input(gpu_ctx):
    """Small, large, small sections (by a 2 KiB limit), with a reader error in the third group."""
    rng = random.Random(21)
    data = gen.fastq(rng, 120, plus_id=0.2)
    rows = _records(gpu_ctx, data)
    small1 = _cut(rng, rows[:30], 1, 4)
    large = [(rows[30][0], rows[70][0] - rows[30][0])]
    small2 = _cut(rng, rows[70:], 1, 4)
    assert large[0][1] > 4096 and all(n <= 2048 for _, n in small1 + small2)
    bad = bytearray(data)
    bad[rows[100][0]] = ord("X")  # record 100 loses its '@'
    return bytes(bad), small1 + large + small2, data, large * 3


def test_stream_both_paths_gpu(gpu_ctx, oracle_lib, monkeypatch):
    """The segmented and the single-section path give the same stream: the limit at 0 (all large), at
    2 KiB (small / large / small, the error in the third group) and at the default (all small)."""
    bad, secs, good, all_large = _mixed_input(gpu_ctx)
    for name in NAMES:
        got = {}
        for limit in ("0", "2048", None):
            if limit is None:
                monkeypatch.delenv("SHOCKIDX_STREAM_SMALL", raising=False)
            else:
                monkeypatch.setenv("SHOCKIDX_STREAM_SMALL", limit)
            r = _check(gpu_ctx, oracle_lib, name, bad, secs)
            got[limit] = (r.gathered, r.count, r.size, r.status, r.err, r.err_section)
            assert r.status == 1 and r.err_section > len(secs) // 2
            _check(gpu_ctx, oracle_lib, name, good, secs)
            _check(gpu_ctx, oracle_lib, name, good, all_large)
        assert got["0"] == got["2048"] == got[None]


def test_stream_anonymize_mixed_formats_gpu(gpu_ctx, oracle_lib):
    """anonymize detects per section: FASTQ, FASTA, FASTQ (the middle one takes the single-section
    path), and a section that detects as nothing (the error at that index)."""
    fq = b"@a\nAC\n+\nII\n@b\nG\n+\nJ\n"
    fa = b">c1 x\nAC\nGT\n>c2\nA\n>c3\nT\n"
    junk = b"hello world\n"
    data = fq + fa + fq + junk + fq
    a, b, c, d = len(fq), len(fq) + len(fa), 2 * len(fq) + len(fa), 2 * len(fq) + len(fa) + len(junk)
    r = _check(gpu_ctx, oracle_lib, "anonymize", data, [(0, a), (a, b - a), (b, c - b)])
    assert r.gathered == b"@1\nAC\n+\nII\n@2\nG\n+\nJ\n>1\nACGT\n>2\nA\n@1\nAC\n+\nII\n@2\nG\n+\nJ\n"
    r = _check(gpu_ctx, oracle_lib, "anonymize", data, [(0, a), (a, b - a), (c, d - c), (d, a)])
    assert (r.err, r.err_section) == (b"Invalid file type for filter", 2)
    _check(gpu_ctx, oracle_lib, "fq2fa", data, [(0, a), (a, b - a), (b, c - b)])  # fq2fa reads FASTA as FASTQ: error
    # a SAM section between FASTQ ones, then one whose alignment line is short (the reader's error)
    from test_oracle_anonymize import ALN, SAM_HEAD
    sam = SAM_HEAD + ALN + b"\n\n" + ALN + b" \n"
    short = SAM_HEAD + ALN + b"\nr2\t0\t*\n" + ALN + b"\n"
    data = fq + sam + fq + short + fq
    e1, e2, e3 = a + len(sam), 2 * a + len(sam), 2 * a + len(sam) + len(short)
    assert oracle_lib.detect(sam)[0] == "sam" and oracle_lib.detect(short)[0] == "sam"
    r = _check(gpu_ctx, oracle_lib, "anonymize", data, [(0, a), (a, len(sam)), (e1, a)])
    assert r.count == 6 and r.err is None
    r = _check(gpu_ctx, oracle_lib, "anonymize", data, [(0, a), (e2, len(short)), (e3, a)])
    assert (r.err, r.err_section, r.count) == (b"sam alignment fields less than 11", 1, 3)


def _device_call(ctx, name, data, secs, cap, fill=0xAB):
    secs = np.asarray(secs, dtype=np.int64).reshape(-1, 2)
    d_in = ctx.alloc(len(data) + 64)
    d_in.upload(data)
    d_secs = ctx.alloc(16 * len(secs) + 64)
    if len(secs):
        d_secs.upload(secs.tobytes())
    d_out = ctx.alloc(cap + 64)
    d_out.fill(fill)
    r = ctx.stream_filter_device(name, d_in.ptr, len(data), d_secs.ptr, len(secs), d_out.ptr, cap)
    return r, d_in, d_secs, d_out


def test_stream_espace_einval_empty_gpu(gpu_ctx, oracle_lib, sample, monkeypatch):
    from shock_amd import _lib as L
    rows = _records(gpu_ctx, sample)
    for limit in (None, "300"):  # one batch; batches and single sections mixed
        if limit:
            monkeypatch.setenv("SHOCKIDX_STREAM_SMALL", limit)
        for name in NAMES:
            exp = streamref.stream_ref(oracle_lib, name, sample, rows)[0]
            r, d_in, d_secs, d_out = _device_call(gpu_ctx, name, sample, rows, len(exp) - 1)
            assert r.status == L.ESPACE and r.size == len(exp)
            assert bytes(d_out.download(len(exp) + 16)) == b"\xab" * (len(exp) + 16)  # nothing written
            r = gpu_ctx.stream_filter_device(name, d_in.ptr, len(sample), d_secs.ptr, len(rows), d_out.ptr, r.size)
            assert r.status == 0 and r.size == len(exp) and r.count == 25 and r.err_section == -1
            got = d_out.download(len(exp) + 16).tobytes()
            assert got[:len(exp)] == exp and got[len(exp):] == b"\xab" * 16
            for b in (d_in, d_secs, d_out):
                b.free()
    for bad in ([(0, 10), (len(sample) - 5, 6)], [(-1, 4)], [(3, -1)], [(len(sample) + 1, 0)]):
        r, *bufs = _device_call(gpu_ctx, "fq2fa", sample, bad, 4096)
        assert r.status == L.EINVAL
        assert bytes(bufs[2].download(64)) == b"\xab" * 64
        for b in bufs:
            b.free()
    for name in NAMES:
        r, *bufs = _device_call(gpu_ctx, name, sample, [], 64)
        assert (r.status, r.count, r.size, r.err_section) == (0, 0, 0, -1)
        for b in bufs:
            b.free()


def test_stream_no_filter_is_gather_gpu(gpu_ctx, sample):
    rows = _records(gpu_ctx, sample)
    secs = [rows[0], rows[3], (rows[7][0], rows[9][0] - rows[7][0])]
    exp = b"".join(sample[p:p + n] for p, n in secs)
    for name in (None, ""):
        r, d_in, d_secs, d_out = _device_call(gpu_ctx, name, sample, secs, len(exp))
        g = gpu_ctx.subset_gather(d_in.ptr, len(sample), d_secs.ptr, len(secs), d_out.ptr, len(exp))
        assert (r.status, r.size, r.err_section) == (0, len(exp), -1) and (g.status, g.size) == (0, r.size)
        assert d_out.download(len(exp)).tobytes() == exp
        for b in (d_in, d_secs, d_out):
            b.free()
    assert gpu_ctx.stream_filter_host(None, sample, secs).gathered == exp


def test_stream_chain_on_device_gpu(gpu_ctx, oracle_lib, sample):
    """subset_node -> idx_range -> stream_filter_device: the runs never visit the host."""
    rows = np.array(_records(gpu_ctx, sample), dtype=np.uint64)
    ids = b"1\n2\n3\n7\n8\n20\n"
    d_ids, d_par, d_data = gpu_ctx.alloc(len(ids) + 64), gpu_ctx.alloc(16 * 25 + 64), gpu_ctx.alloc(len(sample) + 64)
    d_ids.upload(ids)
    d_par.upload(rows.tobytes())
    d_data.upload(sample)
    d_rows, d_runs, d_recs = gpu_ctx.alloc(16 * 8), gpu_ctx.alloc(16 * 8), gpu_ctx.alloc(16 * 8)
    d_gath, d_out = gpu_ctx.alloc(len(sample) + 64), gpu_ctx.alloc(2 * len(sample) + 64)
    sn = gpu_ctx.subset_node(d_ids.ptr, len(ids), d_par.ptr, 25, 25, d_rows.ptr, 8, d_runs.ptr, 8, d_data.ptr,
                             len(sample), d_gath.ptr, len(sample))
    assert sn.ok and sn.count == 6 and sn.runs == 3
    k, err = gpu_ctx.idx_range(d_rows.ptr, sn.count, "1-6", sn.count, d_recs.ptr, 8)
    assert err is None and k == 3
    runs = [(int(o), int(n)) for o, n in d_runs.rows(3)]
    for name in NAMES:
        exp = streamref.stream_ref(oracle_lib, name, sample, runs)
        r = gpu_ctx.stream_filter_device(name, d_data.ptr, len(sample), d_recs.ptr, k, d_out.ptr, 2 * len(sample))
        assert (r.status, r.count, r.size, r.err_section) == (0, exp[1], len(exp[0]), -1)
        assert d_out.download(r.size).tobytes() == exp[0]
    for b in (d_ids, d_par, d_data, d_rows, d_runs, d_recs, d_gath, d_out):
        b.free()


def test_streamer_mirror_gpu(gpu_ctx):
    """request.Streamer: the bytes, then the error; E and ESection (streamer.go:91-96)."""
    from shock_amd import Streamer
    from shock_amd.indexer import ShockIndexError
    node = b"@a\nAC\n+\nII\n@b\nG\n+\nJ\n@c\nGG\n+\nJ\n"
    s = Streamer(R=[(11, 9), (0, 11)], Filter="anonymize")
    assert s.Stream(node).read() == b"@1\nG\n+\nJ\n@1\nAC\n+\nII\n" and s.E is None
    s = Streamer(R=[(0, 11), (11, 19), (0, 11)], Filter="fq2fa")
    rd = s.Stream(node)
    assert rd.read(3) == b">a\n" and rd.read() == b"AC\n>b\nG\n"
    with pytest.raises(ShockIndexError, match="length of sequence and quality"):
        rd.read()
    assert s.ESection == 1 and "length of sequence" in str(s.E)
    assert Streamer(R=[(11, 9), (0, 3)]).Stream(node).read() == b"@b\nG\n+\nJ\n@a\n"
    with pytest.raises(KeyError):
        Streamer(R=[], Filter="gzip")
