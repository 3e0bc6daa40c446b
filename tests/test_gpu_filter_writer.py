"""GPU: the FASTQ filter writer (sidx_filter.hip: k_fq_spans, k_fw_plan, k_fq_write<kind, ORD>) at the
paths no input of test size reaches through the public entry points.

Direct tests (tests/kern.py): a crafted row table and, for anonymize, crafted ordinals ord[] -- record
r's counter is ord[r] + 1 -- go through sidx_filter_spans and sidx_filter_write.  The per-record output
lengths are compared with the reference's first (k_fq_spans alone), then the written bytes, and the 64
bytes past them must keep their 0xAB fill.  The reference is the composition of the oracle's
single-record outputs that tests/test_writer_ref.py proves on the CPU.  Covered: counters of 1 to 10
digits with every 9- and 10-digit run at each of the 16 phases of the 16-byte output chunks, in the
vector path and in the three byte-path arrangements; exactly 512 (sidx_filter_recs()) records per
output block and one byte to either side; thousands of minimal records per block; records whose
output spans three blocks and more.

Not covered: counters of 9 digits and more through k_fq_write<ANON, false> (ord == NULL) need 10^8
records in one section; that instantiation differs from the tested <ANON, true> only in counter().
k_fa_anon_write's counter is the sequence number and cannot be crafted.

Shapes through the public entry points (filter_host with the placed spans and with
SHOCKIDX_FILTER_RESCAN=1, stream_filter_host with the whole input as one section), against the oracle:
a sweep of the output block boundary over every byte of a record, and one whitespace class at each
trimmed edge of a record."""
import random

import numpy as np
import pytest

import kern
import streamref

pytestmark = pytest.mark.gpu
NAMES = ("fq2fa", "anonymize")
ORDS = [0, 8, 9, 98, 99, 99_999_998, 99_999_999, 999_999_998, 999_999_999, 4_294_967_294, 4_294_967_295]
_BASES, _QUALS = b"ACGTN", bytes(range(33, 75))


def _rec(rid: bytes, seq: bytes, qual: bytes, eol=b"\n", plus=b"+") -> bytes:
    assert len(seq) == len(qual)
    return b"@" + rid + eol + seq + eol + plus + eol + qual + eol


def _rand_rec(rng, nseq: int, rid=None) -> bytes:
    """Random bases and qualities (a misplaced record or chunk shows), an ID of 1 to 6 bytes."""
    rid = rid if rid is not None else bytes(rng.choice(b"abcdefghijklmnop") for _ in range(rng.randint(1, 6)))
    return _rec(rid, bytes(rng.choices(_BASES, k=nseq)), bytes(rng.choices(_QUALS, k=nseq)))


def _minimal(rng) -> bytes:
    """@a\\nA\\n+\\nI\\n with the three letters varying."""
    return _rec(bytes([rng.choice(b"abcdefgh")]), bytes([rng.choice(b"ACGT")]), bytes([rng.choice(b"IJKL")]))


def _direct(ctx, oracle, name, recs, ords=None):
    """The pipeline of one direct case -> (outoff, total, wfirst)."""
    kind = kern.KINDS[name]
    counters = [o + 1 for o in ords] if (ords is not None and kind == kern.ANON) else None
    parts = kern.section_ref(oracle, name, recs, counters)
    explen = np.array([len(p) for p in parts], dtype=np.uint64)
    lens = np.array([len(r) for r in recs], dtype=np.uint64)
    rows = np.stack([np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), lens], axis=1)
    case = kern.WriterCase(ctx, b"".join(recs), rows, kind, ords if counters is not None else None)
    try:
        outlen, firstbad = case.spans()
        kern.first_diff(outlen, explen, f"{name}: k_fq_spans output lengths")
        assert firstbad == (1 << 64) - 1
        outoff = np.concatenate([[0], np.cumsum(explen)[:-1]]).astype(np.uint64)
        got, wfirst = case.write(outoff)
    finally:
        case.free()
    exp = b"".join(parts)
    total = len(exp)
    kern.first_diff(np.frombuffer(got[:total], np.uint8), np.frombuffer(exp, np.uint8), f"{name}: output bytes")
    assert got[total:] == b"\xab" * kern.GUARD, f"{name}: wrote past the output"
    return outoff, total, wfirst


def _ndigits(v: int) -> int:
    return len(str(v))


# ---- counter widths ------------------------------------------------------------------------------
def _counter_section():
    """The ORDS list 16 times, each time after a filler record of sequence length 1 ... 16.  In repeat g
    every record of 9 and 10 digits follows one more filler, whose counter width (1 or 2 digits) and
    sequence length are chosen so that the wide record starts at phase g of the 16-byte chunks."""
    rng = random.Random(5)
    recs, ords, cur = [], [], 0

    def add(nseq, o):
        nonlocal cur
        recs.append(_rand_rec(rng, nseq))
        ords.append(o)
        cur += _ndigits(o + 1) + 2 * nseq + 6  # '@' digits '\n' Seq "\n+\n" Qual '\n'

    for g in range(16):
        add(g + 1, g % 9)
        for k, o in enumerate(ORDS):
            if _ndigits(o + 1) >= 9:
                nd, f = next((nd, f) for f in range(1, 9) for nd in (1, 2) if (cur + nd + 2 * f + 6) % 16 == g)
                add(f, 0 if nd == 1 else 10)
            add(1 + (k + g) % 11, o)
    return recs, ords


def _assert_phases(outoff, ords):
    """From outoff: the digit runs (one byte after the record's start) of both widths at all 16 phases."""
    for width in (9, 10):
        ph = {(int(outoff[i]) + 1) % 16 for i, o in enumerate(ords) if _ndigits(o + 1) == width}
        assert ph == set(range(16)), (width, sorted(ph))


def test_counter_widths_every_phase_gpu(gpu_ctx, oracle_lib):
    """Vector path: fw_record's branch for more than 8 digits slices the run per chunk (k0 / k1)."""
    recs, ords = _counter_section()
    assert {_ndigits(o + 1) for o in ORDS} == {1, 2, 3, 8, 9, 10} and max(ORDS) + 1 == 1 << 32
    outoff, total, _ = _direct(gpu_ctx, oracle_lib, "anonymize", recs, ords)
    _assert_phases(outoff, ords)
    assert total < kern.filter_block() and len(recs) < kern.filter_recs()  # all staged: no byte path but the ends
    _direct(gpu_ctx, oracle_lib, "anonymize", recs, None)  # counters r + 1: k_fq_write<ANON, false>
    _direct(gpu_ctx, oracle_lib, "fq2fa", recs, None)


def test_counter_widths_last_record_gpu(gpu_ctx, oracle_lib):
    """Byte path of the last chunk (fw_byte rebuilds the digits with pow10u): each counter as the last
    record, a minimal one, its start at every phase; total % 16 != 0 wherever the last chunk is cut."""
    rng = random.Random(6)
    cut = 0
    for o in ORDS:
        phases = set()
        for p in range(16):
            # two records before the last: 67 output bytes, then nd + 2 f + 6 with (nd, f) chosen for phase p
            nd, f = next((nd, f) for f in range(1, 9) for nd in (1, 2) if (67 + nd + 2 * f + 6) % 16 == p)
            recs = [_rand_rec(rng, 30), _rand_rec(rng, f), _minimal(rng)]
            outoff, total, _ = _direct(gpu_ctx, oracle_lib, "anonymize", recs, [3, 0 if nd == 1 else 10, o])
            phases.add(int(outoff[2]) % 16)
            assert total == int(outoff[2]) + _ndigits(o + 1) + 8
            cut += total % 16 != 0
            if o == ORDS[-1]:
                _direct(gpu_ctx, oracle_lib, "anonymize", recs, None)
                _direct(gpu_ctx, oracle_lib, "fq2fa", recs, None)
        assert phases == set(range(16)), (o, sorted(phases))
    assert cut == 15 * len(ORDS)


def test_counter_widths_first_record_gpu(gpu_ctx, oracle_lib):
    """Record 0: its first run's aligned window would start before the section, so chunk 0 goes byte by byte."""
    rng = random.Random(7)
    for o in ORDS:
        recs = [_rand_rec(rng, 1 + ORDS.index(o) % 4)] + [_rand_rec(rng, 40) for _ in range(3)]
        _direct(gpu_ctx, oracle_lib, "anonymize", recs, [o, 0, 1, 2])
    _direct(gpu_ctx, oracle_lib, "anonymize", recs, None)
    _direct(gpu_ctx, oracle_lib, "fq2fa", recs, None)


def test_counter_widths_past_staged_records_gpu(gpu_ctx, oracle_lib):
    """Byte path beyond the staged records: a block's first sidx_filter_recs() records are minimal ones,
    and the counter list (at every phase again) follows inside the same block."""
    rng = random.Random(8)
    R, block = kern.filter_recs(), kern.filter_block()
    head = [_minimal(rng) for _ in range(R + 5)]
    recs, ords = _counter_section()
    all_recs, all_ords = head + recs, [i % 9 for i in range(len(head))] + ords
    outoff, total, wfirst = _direct(gpu_ctx, oracle_lib, "anonymize", all_recs, all_ords)
    _assert_phases(outoff[len(head):], ords)
    assert total < block and int(outoff[R]) < int(outoff[len(head)])  # one block; the list lies past its staged records
    assert wfirst.tolist() == [0]
    _direct(gpu_ctx, oracle_lib, "anonymize", all_recs, None)
    _direct(gpu_ctx, oracle_lib, "fq2fa", all_recs, None)


# ---- the staging edge: sidx_filter_recs() records per block ------------------------------------------
def _fixed(rng, name, width, count, first_extra=0):
    """count records of exactly `width` output bytes (the first one first_extra bytes more) -> (recs, ords)."""
    recs, ords = [], []
    for i in range(count):
        extra = first_extra if i == 0 else 0
        if name == "fq2fa":  # '>' + 4 ID bytes + '\n' + sequence + '\n'
            nseq, o = width - 7 + extra, 0
            rid = bytes(rng.choices(b"abcdefghij", k=4))
        else:  # '@' + digits + '\n' + sequence + "\n+\n" + quality + '\n' = nd + 2 nseq + 6
            nd = {64: 2, 63: 3, 65: 1}[width]
            nseq = (width - 6 - nd) // 2
            lo, hi = 10 ** (nd - 1), 10 ** nd - 1  # the counters of nd digits
            o = rng.randint(lo, hi) - 1
            if extra:
                assert extra == 1 and nd == 2
                o = rng.randint(100, 999) - 1
            rid = bytes(rng.choices(b"abcdefghij", k=rng.randint(1, 8)))
        recs.append(_rand_rec(rng, nseq, rid))
        ords.append(o)
    return recs, ords


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("width,extra", [(64, 0), (64, 1), (63, 0), (65, 0)], ids=["64", "64+1", "63", "65"])
def test_staging_edge_gpu(gpu_ctx, oracle_lib, name, width, extra):
    """Fixed-width records of 64, 63 and 65 output bytes for more than three blocks: exactly as many
    records per block as are staged, a few more (the block's last ones past the staged records, on the
    byte path) and a few fewer; the 64-byte run starting on a block boundary and one byte past it."""
    R, block = kern.filter_recs(), kern.filter_block()
    assert R * 64 == block  # what makes 64 bytes the edge
    rng = random.Random(width + extra)
    recs, ords = _fixed(rng, name, width, 3 * R + 40, extra)
    outoff, total, wfirst = _direct(gpu_ctx, oracle_lib, name, recs, ords)
    assert np.array_equal(np.diff(outoff)[1:], np.full(len(recs) - 2, width, np.uint64))
    assert int(outoff[1]) == width + extra and total > 3 * block
    # the records starting in each of the first three blocks: as many as are staged, more, fewer
    per_block = np.diff(np.searchsorted(outoff, np.arange(0, 4 * block, block))).tolist()
    assert len(per_block) == 3
    if width == 64:
        assert per_block == [R, R, R]
        assert int(outoff[R]) == block + extra  # the run starts on the block boundary / one byte past it
    elif width == 63:
        assert all(R < k <= R + 9 for k in per_block), per_block
    else:
        assert all(R - 8 <= k < R for k in per_block), per_block
    assert len(wfirst) == 4 and wfirst[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_minimal_records_three_blocks_gpu(gpu_ctx, oracle_lib, name):
    """Minimal records for three blocks: thousands per block under fq2fa (5 output bytes each), about
    1800 with 10-digit counters under anonymize -- all but the first sidx_filter_recs() of every block
    go through the byte path."""
    rng = random.Random(12)
    block = kern.filter_block()
    pool = [_minimal(rng) for _ in range(97)]
    per = 5 if name == "fq2fa" else 18
    count = 3 * block // per + 50
    recs = [pool[rng.randrange(97)] for _ in range(count)]
    ords = [rng.randint(10 ** 9 - 1, (1 << 32) - 1) for _ in range(count)]
    outoff, total, wfirst = _direct(gpu_ctx, oracle_lib, name, recs, ords)
    assert total > 3 * block and total == per * count
    assert min(np.diff(wfirst).tolist()) > 3 * kern.filter_recs()


# ---- long records ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_long_records_gpu(gpu_ctx, oracle_lib, name):
    """Records whose output spans three blocks and more (wfirst names the same record for consecutive
    blocks, which then stage that record alone): one between two dense stretches of minimal records,
    two back to back, and one that starts in a block whose staged records are all minimal ones."""
    rng = random.Random(13)
    R, block = kern.filter_recs(), kern.filter_block()
    nseq = 3 * block + 5 if name == "fq2fa" else (3 * block + 5) // 2 + 1
    long1, long2, long3 = (_rand_rec(rng, nseq + k) for k in range(3))
    dense = lambda k: [_minimal(rng) for _ in range(k)]
    # (records, index of a long record, whether it lies past its block's staged records)
    cases = [(dense(100) + [long1] + dense(R + 90), 100, False),
             (dense(40) + [long1, long2] + dense(40), 41, False),
             (dense(R + 90) + [long3] + dense(10), R + 90, True)]
    for recs, at, past in cases:
        ords = [rng.randrange(0, 99) for _ in recs]
        outoff, total, wfirst = _direct(gpu_ctx, oracle_lib, name, recs, ords)
        out_at = int(outoff[at + 1] - outoff[at]) if at + 1 < len(recs) else total - int(outoff[at])
        assert out_at >= 3 * block + 5
        assert wfirst.tolist().count(at) >= 3  # the same record first in consecutive blocks
        start = int(outoff[at]) // block * block
        r0 = int(np.searchsorted(outoff, start, side="right")) - 1  # the record holding the block's first byte
        assert (at - r0 >= R) == past, (at, r0)
        _direct(gpu_ctx, oracle_lib, name, recs, None)


# ---- shapes through the public entry points ----------------------------------------------------------
def _public(ctx, oracle, name, data, monkeypatch):
    """filter_host with the placed spans and with the rescan, and the stream over one section: the
    oracle's bytes, count, status and error text.  -> the records delivered"""
    out, count, err = oracle.filter_fastq(data, name)
    for rescan in (False, True):
        if rescan:
            monkeypatch.setenv("SHOCKIDX_FILTER_RESCAN", "1")
        else:
            monkeypatch.delenv("SHOCKIDX_FILTER_RESCAN", raising=False)
        r = ctx.filter_host(name, data)
        assert r.status == (0 if err is None else 1), (name, rescan, r.status, r.err, err)
        assert (r.count, r.err, r.size) == (count, err, len(out)), (name, rescan, r.count, r.err, count, err)
        assert r.gathered == out, (name, rescan)
    monkeypatch.delenv("SHOCKIDX_FILTER_RESCAN", raising=False)
    secs = [(0, len(data))]
    exp = streamref.stream_ref(oracle, name, data, secs)
    assert exp[:3] == (out, count, err)
    r = ctx.stream_filter_host(name, data, secs)
    assert r.status == (0 if err is None else 1), (name, "stream", r.status, r.err, err)
    assert (r.gathered, r.count, r.err, r.err_section) == exp, (name, "stream", r.count, r.err, exp[1:])
    return count


def _literals(name, out2):
    """[(first byte, one past the last)] of the literals in one record's output."""
    n = len(out2)
    if name == "fq2fa":  # '>' ID '\n' Seq '\n'
        k = out2.index(b"\n")
        return [(0, 1), (k, k + 1), (n - 1, n)]
    k = out2.index(b"\n+\n")  # "@digits\n" Seq "\n+\n" Qual '\n'
    return [(0, out2.index(b"\n") + 1), (k, k + 3), (n - 1, n)]


@pytest.mark.parametrize("name", NAMES)
def test_block_seam_sweep_gpu(gpu_ctx, oracle_lib, monkeypatch, name):
    """A first record of sequence length F and three short ones (one with CRLF, one with a "+id" line);
    F steps by 1 over 80 values so that the first output block's end passes over every byte of the
    second record's output and the first byte of the third's.  Under anonymize one step of F moves the
    boundary by two bytes and every record's output among the first nine has an odd length, so the
    sweep runs a second time behind one more leading record: the other parity."""
    block = kern.filter_block()
    rng = random.Random(14)
    seq, qual = bytes(rng.choices(_BASES, k=block)), bytes(rng.choices(_QUALS, k=block))
    short = [_rec(b"s2 x", b"ACGTAC", b"IJKLMN", eol=b"\r\n"), _rec(b"s3", b"GGT", b"abc", plus=b"+s3"),
             _rec(b"s4", b"T", b"!")]
    first = lambda F: _rec(b"f", seq[:F], qual[:F])
    covered, need = set(), set()
    for lead in ([], [_rec(b"l", b"C", b"#")]) if name == "anonymize" else ([],):
        n0 = len(lead)
        ref = lambda r, i: kern.record_ref(oracle_lib, name, r, i + 1)
        lead_out = sum(len(ref(r, i)) for i, r in enumerate(lead))
        base = len(ref(first(1), n0))
        step = len(ref(first(2), n0)) - base
        out2 = ref(short[0], n0 + 1)
        assert step == (1 if name == "fq2fa" else 2) and len(out2) + 2 <= 80
        # d(F): where the block ends inside the second record's output (0: before its first byte)
        d = lambda F: block - lead_out - base - step * (F - 1)
        # the 80 values end at d = 0 (or 1, by parity): past that the first record would outgrow the 32 KiB
        # that the format detection reads
        top = 79 * step + (d(1) - 79 * step) % step
        F0 = 1 + (d(1) - top) // step
        assert d(F0) == top >= len(out2) + 1 and d(F0 + 79) in (0, 1)
        for lo, hi in _literals(name, out2):
            need |= set(range(lo, hi + 1))
        need.add(len(out2) + 1)  # the boundary after the third record's first byte
        for F in range(F0, F0 + 80):
            assert _public(gpu_ctx, oracle_lib, name, b"".join(lead + [first(F)] + short), monkeypatch) == n0 + 4
            covered.add(d(F))
    assert need <= covered, sorted(need - covered)  # every literal straddles the boundary at some F


_WS = [b" ", b"\t", b"\r", b"\v", b"\f", "\u0085".encode(), "\u00a0".encode(), "\u2003".encode(),
       "\u3000".encode(), b"\x85", b"\xc2", "\u200b".encode(), b"\x7f", b"\x00"]
_EDGES = {"id-left": "I", "id-right": "i", "seq-left": "S", "seq-right": "s", "qual-left": "Q", "qual-right": "q",
          "seq+qual-left": "SQ", "seq+qual-right": "sq", "all-six": "IiSsQq"}


def _edge_record(ws: bytes, edges: str) -> bytes:
    e = lambda c: ws if c in edges else b""
    return (b"@" + e("I") + b"odd" + e("i") + b"\n" + e("S") + b"ACGT" + e("s") + b"\n+\n" + e("Q") + b"IJKL" + e("q")
            + b"\n")


@pytest.mark.parametrize("name", NAMES)
def test_edge_byte_matrix_gpu(gpu_ctx, oracle_lib, monkeypatch, name):
    """One whitespace class at one trimmed edge of the middle record of clean + odd + clean: 14 classes
    (ASCII spaces, Unicode spaces as UTF-8, the bare bytes 0x85 and 0xC2, and three bytes that are no
    spaces) at 9 placements.  The oracle decides every case; most deliver all three records (the fast
    path's seven edge bytes against trim_space), the rest end in Read's error after the first."""
    clean1, clean2 = _rec(b"c1 x", b"ACGTT", b"IIIII"), _rec(b"c2", b"GG", b"JJ", plus=b"+c2")
    three = 0
    for ws in _WS:
        for edges in _EDGES.values():
            three += _public(gpu_ctx, oracle_lib, name, clean1 + _edge_record(ws, edges) + clean2, monkeypatch) == 3
    assert len(_WS) * len(_EDGES) == 126 and three >= 100, three
