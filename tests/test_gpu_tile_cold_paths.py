"""GPU: the branches of the FASTQ and FASTA tile passes (k_fq_tiles, k_fa_tiles) that a clean
short-read file never takes, each on a constructed input of 2 to 40 tiles built through the public
build and compared -- whole table, count, error text -- with the oracle; the FASTQ inputs also
through fq2fa, whose spans come from k_fq_tiles<true>.

These branches read what they need off the kernel arguments where they run, and the tile's bounds
are offsets from its claim's first byte, so each case is placed where that matters: in tile 0, in a
claim's later tiles and in the slab's last tile.  Already pinned elsewhere and not repeated here:
CRLF and every structural byte at a tile seam, records past the halo, IDs of 63-700 bytes at the
lane / wave-cooperative edge, MAX_DEFER, 63-65 records per tile and the overflow slot, tiles past
SNLCAP - NLHALO, the FASTQ file end at every length mod 4 (tests/test_gpu_fastq_tiles.py); claims
that end on a burst shorter than FQ_BLK (tests/test_gpu_tile_claim.py).  A FASTQ tile of more than
RCAP = 256 records has more than 1020 '\\n' and is past SNLCAP - NLHALO already: that branch has no
input of its own.  A tile with fewer than FRONT bytes in front of it is every file's tile 0."""
import random

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

TILE, HALO, FRONT = 16384, 1024, 16
ID_MISMATCH = b"Invalid format: quality ID does not match sequence ID"


def _same(r, rows, err, what):
    assert r.count == len(rows), (what, r.count, len(rows), r.err, err)
    assert r.err == err, (what, r.err, err)
    got = r.rows if r.rows is not None else np.zeros((0, 2), np.uint64)
    if not np.array_equal(got, rows):
        bad = np.nonzero((got != rows).any(axis=1))[0][:5]
        raise AssertionError(f"{what}: first mismatching rows {bad.tolist()}: gpu {got[bad].tolist()} "
                             f"oracle {rows[bad].tolist()}")


def _record(ctx, oracle_lib, data, fmt, what):
    rows, err = oracle_lib.record_index(data, fmt)
    r = ctx.build_host(data, kind="record", fmt=fmt)
    _same(r, rows, err, what)
    assert (r.path, r.reruns) == (1, 0), (what, r.path, r.reruns)
    return rows, err


def _fq2fa(ctx, oracle_lib, data, what):
    out, n, err = oracle_lib.filter_fastq(data, "fq2fa")
    r = ctx.filter_host("fq2fa", data)
    assert r.status in (0, 1), (what, r.status, r.err)
    assert (r.count, r.err) == (n, err), (what, r.count, r.err, n, err)
    assert r.gathered == out, what


# ---- the 3-instruction '\n' flags and their exact re-check ------------------------------------------
# eq4x flags a byte equal to the pattern, and also pattern ^ 1 right above a flagged byte of the same
# dword: "\n\v" ('\v' = '\n' ^ 1) and ">?" ('?' = '>' ^ 1).  eq_suspect sees two flags side by side in
# a dword and the word is classified again exactly.  A thread reads its 64-byte word as four 16-byte
# chunks; the pair is put in each chunk, at each place of a dword it fits, and for FASTQ also in the
# first bytes past a tile's end, which the owner's last wave classifies from the halo.
PAIR_AT = [16 * c + 4 * (c % 3 + 1) + k for c in range(4) for k in range(3)]  # offsets in a 64-byte word


def _fq_vt_file(pos, ntiles=3):
    """fq_fill with one record '@id / \\vACGT... / + / IIII...' whose ID line ends at byte pos: Go
    trims the '\\v' (a valid record, never certified by the tile: k_fixup validates it)."""
    rid = gen.fq_id(9, pos)
    probe = b"@" + rid + b"\n\v" + b"ACGT" * 10 + b"\n+\n" + b"I" * 40 + b"\n"
    start = pos - 1 - len(rid)
    total = (ntiles - 1) * TILE + 6000
    data = gen.fq_fill(start) + probe + gen.fq_fill(total - start - len(probe))
    assert data[pos:pos + 2] == b"\n\v" and len(data) == total
    return data


def test_fastq_suspect_pairs_gpu(gpu_ctx, oracle_lib):
    for tile, word in ((0, 9), (1, 201), (2, 5)):
        for off in PAIR_AT:
            pos = tile * TILE + 64 * word + off
            what = f"fastq '\\n\\v' at tile {tile} word {word} byte {off}"
            data = _fq_vt_file(pos)
            rows, err = _record(gpu_ctx, oracle_lib, data, "fastq", what)
            assert err is None and len(rows) > 60, what
    for k in range(3):  # in the halo of tile 0 / tile 1: one of the first four '\n' past the tile's end
        for tile in (1, 2):
            pos = tile * TILE + 4 + k
            what = f"fastq '\\n\\v' in the halo, {4 + k} bytes past tile {tile - 1}"
            data = _fq_vt_file(pos)
            _record(gpu_ctx, oracle_lib, data, "fastq", what)
            _fq2fa(gpu_ctx, oracle_lib, data, what)
    _fq2fa(gpu_ctx, oracle_lib, _fq_vt_file(TILE + 64 * 201 + PAIR_AT[4]), "fq2fa '\\n\\v' in a word")


def _fa_pair_file(pos, pair, ntiles=3):
    """60-byte FASTA records with the pair at byte pos: ">?" opens a record whose header starts with
    '?', "\\n\\v" is inside a record's sequence."""
    rec = lambda i: b">r%06d\n" % i + b"ACGTACGTAC" * 5 + b"\n"
    probe = (b">?hdr\n" + b"ACGT" * 6 + b"\n") if pair == b">?" else b">h\nACGT\n\vACGT\n"
    start = pos - probe.index(pair)
    head = b"".join(rec(i) for i in range((start - 70) // 60))
    head += b">p\n" + b"A" * (start - len(head) - 4) + b"\n"  # a record that ends where the probe starts
    nrest = ((ntiles - 1) * TILE + 5001 - start - len(probe)) // 60
    data = head + probe + b"".join(rec(i) for i in range(nrest))
    assert len(rec(0)) == 60 and len(head) == start and data[pos:pos + 2] == pair
    return data


@pytest.mark.parametrize("pair", [b">?", b"\n\v"], ids=["gt", "nl"])
def test_fasta_suspect_pairs_gpu(gpu_ctx, oracle_lib, pair):
    for tile, word in ((0, 9), (1, 201), (2, 5)):
        for off in PAIR_AT:
            pos = tile * TILE + 64 * word + off
            what = f"fasta {pair!r} at tile {tile} word {word} byte {off}"
            rows, err = _record(gpu_ctx, oracle_lib, _fa_pair_file(pos, pair), "fasta", what)
            assert err is None and len(rows) > 500, what


# ---- the slab's last tile: zero fill, the tail dword, the EOF piece ------------------------------------
@pytest.mark.parametrize("ntiles", [2, 33, 40])
def test_fasta_slab_end_lengths_gpu(gpu_ctx, oracle_lib, ntiles):
    """Files of ntiles tiles whose last tile holds 1, 2, 3 bytes, and 4093 .. 4099: every length mod 4
    (the DMA's range check drops a partial last dword, tail_dword / patch_tail fetch its bytes), with
    the last '\\n' present and cut off, and with the EOF piece valid and without a '\\n' at all
    (fasta.go:111-125).  33 tiles: the last tile opens a claim; 40: it ends one."""
    body = gen.fasta(random.Random(ntiles), 20 * ntiles + 40, embedded_gt=0.05)
    assert len(body) > ntiles * TILE
    for r in (1, 2, 3, 4093, 4094, 4095, 4096, 4097, 4098, 4099):
        n = (ntiles - 1) * TILE + r
        cut = body[:n]
        for tail in (b"", b"\n", b">x", b">xy\nAC"):
            data = cut[:n - len(tail)] + tail
            assert len(data) == n
            _record_any(gpu_ctx, oracle_lib, data, "fasta", f"fasta end ntiles={ntiles} r={r} tail={tail!r}")


def _record_any(ctx, oracle_lib, data, fmt, what):
    """As _record for an input that may end in Go's error."""
    rows, err = oracle_lib.record_index(data, fmt)
    r = ctx.build_host(data, kind="record", fmt=fmt)
    _same(r, rows, err, what)
    assert r.path == 1, (what, r.path, r.reruns)
    return rows, err


@pytest.mark.parametrize("ntiles", [2, 33])
def test_fastq_slab_end_lengths_gpu(gpu_ctx, oracle_lib, ntiles):
    """The same lengths for FASTQ where a claim boundary is the last tile's start (33 tiles), and
    through fq2fa: a last record cut inside its quality line is still a record (EOF tolerated)."""
    for r in (1, 2, 3, 4097, 4098, 4099):
        n = (ntiles - 1) * TILE + r
        data = gen.fq_fill(n + 700)[:n]
        what = f"fastq end ntiles={ntiles} r={r}"
        _record_any(gpu_ctx, oracle_lib, data, "fastq", what)
        _fq2fa(gpu_ctx, oracle_lib, data, what)


# ---- plus-line IDs at the lane / wave edge, in a claim's later tiles -------------------------------------
@pytest.mark.parametrize("nid", [64, 65, 300])
def test_fastq_plus_ids_gpu(gpu_ctx, oracle_lib, nid):
    """An ID of 64 bytes (one lane compares it), 65 and 300 (the whole wave does), repeated on the plus
    line, in tile 0 (the file-start variant of the position reads) and in tile 17 (the second burst of
    a claim): equal, and with the copy's last byte changed -- Go's ID mismatch after the records in
    front.  Equal ones also through fq2fa."""
    for tile in (0, 17):
        for flip in (False, True):
            lines = gen.fq_lines(nid, 30, plus_id=True, tag=nid)
            if flip:
                c = b"#" if lines[2][-2:-1] != b"#" else b"%"
                lines[2] = lines[2][:-2] + c + b"\n"
            rec = b"".join(lines)
            start = tile * TILE + 1024
            data = gen.fq_fill(start) + rec + gen.fq_fill(19 * TILE + 5000 - start - len(rec))
            what = f"plus id nid={nid} tile={tile} flip={flip}"
            rows, err = _record_any(gpu_ctx, oracle_lib, data, "fastq", what)
            if flip:
                assert (len(rows), err) == (start // 512, ID_MISMATCH), (what, len(rows), err)
            else:
                assert err is None, (what, err)
                _fq2fa(gpu_ctx, oracle_lib, data, what)


# ---- dense tiles ---------------------------------------------------------------------------------------
def test_dense_tiles_gpu(gpu_ctx, oracle_lib):
    """FASTA: more candidates than a tile's table holds (RCAP = 256) in tiles 1 and 34 of 36, the
    rest sparse.  FASTQ: 100 space-padded records (never certified: more than MAX_DEFER) in tile 1,
    and a tile of 60-byte records (more '\\n' than SNLCAP - NLHALO) as tile 34, both whole-tile items
    for k_fixup next to certified tiles of the same claim."""
    sparse = b"".join(b">s%05d\n" % i + b"ACGT" * 30 + b"\n" for i in range(40 * TILE // 128 + 1))
    dense = b"".join(b">d%03d\nAC\n" % (i % 1000) for i in range(TILE // 8 + 8))
    cut = lambda b, n: b[:b.rfind(b"\n>", 0, n) + 1]
    parts, size = [], 0
    for t0, src in ((TILE, sparse), (2 * TILE, dense), (34 * TILE, sparse), (35 * TILE, dense), (36 * TILE - 77, sparse)):
        p = cut(src, t0 - size)
        parts.append(p)
        size += len(p)
    data = b"".join(parts)
    rows, err = _record(gpu_ctx, oracle_lib, data, "fasta", "fasta dense tiles")
    assert err is None and len(rows) > 2 * (TILE // 8)
    pad = gen.fq_rec(7, 33, pad=b" ")
    fq = gen.fq_fill(TILE) + pad * 100
    fq += gen.fq_fill(34 * TILE - len(fq)) + gen.fq_uniform(60, TILE)
    fq += gen.fq_fill(36 * TILE - 77 - len(fq))
    rows, err = _record(gpu_ctx, oracle_lib, fq, "fastq", "fastq dense tiles")
    assert err is None
    _fq2fa(gpu_ctx, oracle_lib, fq, "fastq dense tiles")
