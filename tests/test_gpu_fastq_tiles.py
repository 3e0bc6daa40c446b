"""GPU parity of the FASTQ tile pass (k_fq_tiles -> k_scan_excl -> k_fq_place -> k_fixup) against
the oracle, at the edges of its own mechanisms (fastq.go:134-213 semantics, oracle/shockidx_oracle.c).

A tile certifies from LDS every record it owns (the record after each fourth '\\n' in it) whose
closing '\\n' it sees (the tile plus SHALO = HALO - FRONT bytes past it), and sends the rest to
k_fixup: a record it cannot certify as one queue item each (up to MAX_DEFER per tile), a tile of too
many lines, too many such records or a misread phase as one whole-tile item.  (A file that ends in
a whole record always queues one item: the record that would start at its end, which k_fixup finds
absent.)  The records' starts leave in a 64-entry line per tile plus an overflow slot, in bursts of
16 tiles, in batches of 32 tiles per workgroup; k_fq_place stages 64 tiles' entries in LDS
(PLACE_ECAP) or places tile by tile.  Every corpus here is constructed
(tests/gen.py: fq_rec / fq_fill / fq_uniform) so that one of these edges is hit on purpose, and a case
that names its mechanism runs on a context of its own and asserts through path / reruns / fixups /
fix_tiles that the mechanism was reached: the fix-up queue's capacity grows with a context's history,
so the session's shared context would make those counters depend on the test order."""
import contextlib

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

# the tile pass's constants (sidx_common.hpp, sidx_kernels.hip)
TILE, HALO, FRONT = 16384, 1024, 16
SHALO = HALO - FRONT        # bytes past the tile a slot holds: position TILE + SHALO is the first not seen
NLHALO, SNLCAP = 4, 1024    # a tile is fast while its '\n' count + NLHALO <= SNLCAP
MAX_DEFER = 16
PLACE_TILES, PLACE_ECAP = 64, 8192
ID_MISMATCH = b"Invalid format: quality ID does not match sequence ID"


@contextlib.contextmanager
def _fresh():
    """A context of this case alone: its fix-up queue holds what ensure_tiles gives this file."""
    from shock_amd import Context
    ctx = Context(0)
    try:
        yield ctx
    finally:
        ctx.close()


def _check(ctx, oracle_lib, data, fmt="fastq", what=""):
    r = ctx.build_host(data, kind="record", fmt=None if fmt == "auto" else fmt)
    rows, err = oracle_lib.record_index(data, None if fmt == "auto" else fmt)
    assert r.count == len(rows), (what, r.count, len(rows), r.err, err)
    assert r.err == err, (what, r.err, err)
    got = r.rows if r.rows is not None else np.zeros((0, 2), np.uint64)
    if not np.array_equal(got, rows):
        bad = np.nonzero((got != rows).any(axis=1))[0][:5]
        raise AssertionError(f"{what}: first mismatching rows {bad.tolist()}: gpu {got[bad].tolist()} "
                             f"oracle {rows[bad].tolist()}")
    return r, rows


def _tile_pass(r, what):
    assert (r.path, r.reruns) == (1, 0), (what, r.path, r.reruns, r.fixups, r.fix_tiles)


def _owner(rows):
    """The tile that certifies each record: the one holding the '\\n' before its start (a record that
    starts on a tile's first byte belongs to the tile before), tile 0 for record 0."""
    st = rows[:, 0].astype(np.int64)
    return np.maximum(st - 1, 0) // TILE


def _expect_fix(data, rows):
    """(fixups, fix_tiles) the tile pass owes a valid file without padded lines, mirrored from
    tiles_iter and k_fq_place.  A tile goes to k_fixup whole when it has more than SNLCAP - NLHALO
    '\\n', when the phase read off its first 16 '\\n' (fq_guess_at; tile 0's is known) is none or not
    the true one, or when it defers more than MAX_DEFER records.  Otherwise it defers the records it
    owns whose closing '\\n' lies at or past TILE + SHALO of its start -- and, in the tile that holds
    the file's last '\\n', the record that would start at the file's end."""
    a = np.frombuffer(data, np.uint8)
    nt = -(-len(a) // TILE)
    nl = np.flatnonzero(a == 10)
    T = np.bincount(nl // TILE, minlength=nt)
    rank = np.concatenate(([0], np.cumsum(T)))  # '\n' before each tile
    whole = T + NLHALO > SNLCAP
    for t in range(1, nt):
        if whole[t]:
            continue
        vis = nl[rank[t]:rank[t] + T[t] + NLHALO]
        vis = vis[vis < t * TILE + TILE + SHALO]
        guess = None
        for c in range(min(16, max(len(vis) - 4, 0))):
            p0, p1, p2, p3, p4 = (int(x) for x in vis[c:c + 5])
            if a[p0 + 1] == 0x40 and a[p2 + 1] == 0x2B and p2 - p1 > 1 and p2 - p1 == p4 - p3:
                guess = c & 3
                break
        true = (3 - (int(rank[t]) & 3)) & 3
        groups = lambda g: (T[t] - g + 3) // 4 if g < T[t] else 0
        whole[t] = guess is None or (guess != true and (groups(true) | groups(guess)) != 0)
    own = _owner(rows)
    far = rows[:, 0].astype(np.int64) + rows[:, 1].astype(np.int64) - 1 - own * TILE >= TILE + SHALO
    defer = np.bincount(own[far], minlength=nt)
    if len(a) and a[-1] == 10 and len(nl) % 4 == 0:
        defer[(len(a) - 1) // TILE] += 1
    whole |= defer > MAX_DEFER
    return int(whole.sum() + defer[~whole].sum()), int(whole.sum())


def _fixcap(ntiles):
    """ensure_tiles (sidx_build.cpp): a context's first build of ntiles tiles allocates
    ntiles + ntiles / 8 + 64 status words per array, and the k_fixup queue holds as many items."""
    return ntiles + ntiles // 8 + 64


def _place_entries(rows, ntiles):
    """k_fq_place step 1: a placed tile stages (nrec + 8) / 8 chunks of 8 u16 entries (its starts and
    the last record's end); E per 64-tile workgroup run."""
    nrec = np.bincount(_owner(rows), minlength=ntiles)
    ent = np.where(nrec > 0, (nrec + 8) // 8, 0) * 8
    pad = np.zeros(-(-ntiles // PLACE_TILES) * PLACE_TILES, np.int64)
    pad[:ntiles] = ent
    return pad.reshape(-1, PLACE_TILES).sum(axis=1)


def _marks(lines):
    """Offsets in a record of its five structural bytes: the '@' and the four '\\n'."""
    out, o = [0], 0
    for ln in lines:
        o += len(ln)
        out.append(o - 1)
    return out


# ---- 1. one probe record, every structural byte moved across a tile end ---------------------------
VARIANTS = [(eol, plus_id, qual_at) for eol in (b"\n", b"\r\n") for plus_id in (False, True)
            for qual_at in (False, True)]
THIN = [(b"\n", False, False), (b"\r\n", True, True)]
SEAM_TILES = 66
SEAMS = {"plain": 1, "burst": 16, "batch": 32, "group": 64}


def _seam_file(k, mark, d, lines, ntiles=SEAM_TILES):
    """fq_fill + probe + fq_fill over ntiles tiles with the probe's mark at k TILE + d."""
    probe = b"".join(lines)
    start = k * TILE + d - _marks(lines)[mark]
    total = (ntiles - 1) * TILE + 6000  # (a last tile of a dozen records: its phase is visible)
    data = gen.fq_fill(start) + probe + gen.fq_fill(total - start - len(probe))
    assert len(data) == total and data[start:start + len(probe)] == probe
    return data


@pytest.mark.parametrize("seam", sorted(SEAMS))
def test_fastq_seam_sweep_gpu(oracle_lib, seam):
    """The probe's '@' and each of its four '\\n' at d = -3 .. +3 of the end of tile k - 1: a plain
    tile end, a store burst's end (16), a batch's end (32: the halo is another workgroup's tile) and
    a placement group's end (64); LF and CRLF (at d = 0 the '\\r' is the tile's last byte), a bare
    plus line and one with the ID, a quality line that starts with '@'.  The probe lies within the
    halo of the tile that owns it: certified there, so k_fixup gets the file's end and nothing else."""
    k = SEAMS[seam]
    with _fresh() as ctx:
        for eol, plus_id, qual_at in VARIANTS:
            lines = gen.fq_lines(11, 40, eol=eol, plus_id=plus_id, qual_at=qual_at, tag=k)
            for mark in range(5):
                for d in range(-3, 4):
                    what = f"seam k={k} mark={mark} d={d} eol={eol!r} plus_id={plus_id} qual_at={qual_at}"
                    data = _seam_file(k, mark, d, lines)
                    r, rows = _check(ctx, oracle_lib, data, "fastq", what)
                    _tile_pass(r, what)
                    assert _expect_fix(data, rows) == (1, 0), what  # the file's end alone
                    assert (r.fixups, r.fix_tiles) == (1, 0), (what, r.fixups, r.fix_tiles)


def _fs_lines(mark, d, eol, plus_id, qual_at):
    """Record 0 of a file with its mark (1-4) at offset TILE + d: the line before the mark is long."""
    e, p, nid, nseq = len(eol), int(plus_id), 6, 20
    target = TILE + d
    if mark == 1:
        nid = target - e
    elif mark == 2:
        nseq = target - (nid + e) - e
    elif mark == 3:
        nseq = target - (nid + e) - e - 1 - p * nid - e
    else:
        rest = target - (nid + e) - 1 - p * nid - 3 * e
        if rest % 2:
            if plus_id:  # 2 nid + 2 nseq + 1 + 4 e: this offset has the wrong parity for any record
                return None
            nid, rest = nid + 1, rest - 1
        nseq = rest // 2
    lines = gen.fq_lines(nid, nseq, eol=eol, plus_id=plus_id, qual_at=qual_at)
    assert _marks(lines)[mark] == target
    return lines


def test_fastq_seam_file_start_gpu(oracle_lib):
    """The same marks with the probe as record 0 of the file, crossing tile 0's end (file_start:
    record 0 has no '\\n' before it).  Such a record is 16 to 33 KiB long, so whether it is
    certified, queued alone or leaves a tile without a visible phase behind it differs per case:
    _expect_fix says which."""
    with _fresh() as ctx:
        for eol, plus_id, qual_at in VARIANTS:
            for mark in range(1, 5):
                for d in range(-3, 4):
                    lines = _fs_lines(mark, d, eol, plus_id, qual_at)
                    if lines is None:
                        continue
                    what = f"file start mark={mark} d={d} eol={eol!r} plus_id={plus_id} qual_at={qual_at}"
                    probe = b"".join(lines)
                    data = probe + gen.fq_fill(4 * TILE + 6000 - len(probe))
                    r, rows = _check(ctx, oracle_lib, data, "fastq", what)
                    _tile_pass(r, what)
                    assert rows[0, 1] == len(probe), what
                    want = _expect_fix(data, rows)
                    assert (r.fixups, r.fix_tiles) == want, (what, r.fixups, r.fix_tiles, want)


@pytest.mark.parametrize("seam", sorted(SEAMS))
def test_fastq_seam_invalid_gpu(oracle_lib, seam):
    """The seam sweep's probe made invalid in each of Go's ways, at d = -1, 0, +1 of every mark: the
    records before it and Go's error text.  The probe is never certified: k_fixup reports it."""
    k = SEAMS[seam]
    with _fresh() as ctx:
        for eol, plus_id, qual_at in THIN:
            for bad in gen.FQ_BAD:
                lines = gen.fq_lines(11, 40, eol=eol, plus_id=plus_id, qual_at=qual_at, tag=k, bad=bad)
                for mark in range(5):
                    for d in (-1, 0, 1):
                        what = f"invalid {bad} k={k} mark={mark} d={d} eol={eol!r} plus_id={plus_id}"
                        data = _seam_file(k, mark, d, lines)
                        r, rows = _check(ctx, oracle_lib, data, "fastq", what)
                        _tile_pass(r, what)
                        # the probe and the file's end
                        assert r.err is not None and (r.fixups, r.fix_tiles) == (2, 0), (what, r.err, r.fixups, r.fix_tiles)
                        start = k * TILE + d - _marks(lines)[mark]
                        assert len(rows) == start // 512, what  # fq_fill(start): 512-byte records, the last one longer


# ---- 2. the halo limit ----------------------------------------------------------------------------
def _halo_file(k, kind, P):
    """A probe that starts s bytes before the end of tile k - 1 with its fourth '\\n' at offset P of
    that tile; kind names the long line(s)."""
    s = {"id": 20, "plus": 20, "seq": 600, "qual": 4}[kind]
    if kind == "plus" and (P - TILE + s + 1) % 2:  # a record with the ID twice has an even length
        s += 1
    n = P - (TILE - s) + 1
    if kind == "id":
        probe = gen.fq_sized(n, nseq=20, tag=P)
    elif kind == "plus":
        probe = gen.fq_sized(n, nseq=20, plus_id=True, tag=P)
    else:  # the sequence and the quality line are equally long: mostly in the tile, or all past it
        probe = gen.fq_sized(n, tag=P)
    start = k * TILE - s
    total = (k + 1) * TILE + 5000
    data = gen.fq_fill(start) + probe + gen.fq_fill(total - start - n)
    assert data[(k - 1) * TILE + P] == 10 and data[start] == 64 and len(data) == total
    return data


@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("kind", ["id", "plus", "seq", "qual"])
def test_fastq_halo_limit_gpu(oracle_lib, kind, k):
    """The probe's closing '\\n' swept over offsets TILE + 990 .. TILE + 1030 of the tile it starts
    in.  A slot holds SHALO = HALO - FRONT = 1008 bytes past its tile, so TILE + 1007 is the last
    position seen: the record is certified up to there and is one k_fixup item from TILE + 1008 on.
    At k = 32 the probe's tile ends a batch: its halo is the first KiB of another workgroup's tile."""
    with _fresh() as ctx:
        got = []
        for P in range(TILE + 990, TILE + 1031):
            what = f"halo kind={kind} k={k} P=TILE+{P - TILE}"
            data = _halo_file(k, kind, P)
            r, rows = _check(ctx, oracle_lib, data, "fastq", what)
            _tile_pass(r, what)
            assert r.fix_tiles == 0, (what, r.fix_tiles)
            assert r.fixups == _expect_fix(data, rows)[0], (what, r.fixups)
            got.append(r.fixups - 1)  # (less the file's end)
        step = TILE + SHALO - (TILE + 990)
        assert got == [0] * step + [1] * (len(got) - step), (kind, k, got)


# ---- 3. plus-line IDs longer than a lane compares alone -------------------------------------------
IDLENS = [63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 258, 259, 260, 511, 512, 513, 700]


def _longid_file(nid, shift, eol, flip=None):
    """A first record of 512 + shift bytes, then a record with an nid-byte ID repeated on its plus
    line (one byte of the copy changed when flip is given), then filler: two tiles."""
    first = gen.fq_sized(512 + shift)
    lines = gen.fq_lines(nid, 30, eol=eol, plus_id=True, tag=nid)
    if flip is not None:
        pl = bytearray(lines[2])
        assert pl[1 + flip] != 0x23
        pl[1 + flip] = 0x23
        lines[2] = bytes(pl)
    rec = b"".join(lines)
    assert len(first) + len(rec) < TILE + SHALO
    return first + rec + gen.fq_fill(2 * TILE - 200 - len(first) - len(rec))


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_fastq_long_plus_id_gpu(oracle_lib, eol):
    """IDs around 64 bytes (one lane compares up to 64) and around the wave-cooperative loop's
    256-byte stride, at the four byte alignments of the record.  Equal: certified from LDS, only the
    file's end for k_fixup.  One byte of the copy changed -- the first, byte 63, 64, 255, 256, the
    last: Go's ID mismatch after one record."""
    with _fresh() as ctx:
        for nid in IDLENS:
            for shift in range(4):
                what = f"long id nid={nid} shift={shift} eol={eol!r}"
                r, rows = _check(ctx, oracle_lib, _longid_file(nid, shift, eol), "fastq", what)
                _tile_pass(r, what)
                assert (r.fixups, r.fix_tiles) == (1, 0), (what, r.fixups, r.fix_tiles)  # the file's end alone
                for flip in sorted({0, 63, 64, 255, 256, nid - 1}):
                    if flip >= nid:
                        continue
                    r, rows = _check(ctx, oracle_lib, _longid_file(nid, shift, eol, flip), "fastq", f"{what} flip={flip}")
                    _tile_pass(r, f"{what} flip={flip}")
                    assert (len(rows), r.err) == (1, ID_MISMATCH), (what, flip, len(rows), r.err)


LONG_AT = {0: 65, 5: 300, 31: 257, 63: 513, 64: 129, 70: 258, 100: 260}  # record tile 1 owns -> ID length


def _dense_longid_file(flip_at=None):
    """Tile 1 starts on a record, which tile 0 owns; the 120 after it are 100 bytes long except those
    of LONG_AT, whose IDs are long and repeated on the plus line (flip_at: that one's copy differs in
    its last byte)."""
    recs = [gen.fq_sized(100, tag=999)]
    for i in range(120):
        if i in LONG_AT:
            lines = gen.fq_lines(LONG_AT[i], 10, plus_id=True, tag=i)
            if i == flip_at:
                lines[2] = lines[2][:-2] + (b"#" if lines[2][-2:-1] != b"#" else b"%") + b"\n"
            recs.append(b"".join(lines))
        else:
            recs.append(gen.fq_sized(100, tag=i))
    body = b"".join(recs)
    return gen.fq_fill(TILE) + body + gen.fq_fill(3 * TILE - 300 - TILE - len(body))


def test_fastq_long_plus_id_lanes_gpu(oracle_lib):
    """Several long-ID records in one dense tile: the cooperative loop serves one lane at a time, so
    they sit in different lanes of the certifying wave (records 0, 5, 31, 63 of those the tile owns)
    and in the tile's second wave (records 64, 70, 100).  All equal: only the file's end for
    k_fixup.  Each one's copy changed in its last byte in turn: Go's ID mismatch, the count the
    records before it."""
    with _fresh() as ctx:
        r, rows = _check(ctx, oracle_lib, _dense_longid_file(), "fastq", "dense long ids")
        _tile_pass(r, "dense long ids")
        assert (r.fixups, r.fix_tiles) == (1, 0), (r.fixups, r.fix_tiles)
        own = _owner(rows)
        assert rows[32, 0] == TILE and own[32] == 0 and (own[33:33 + 120] == 1).all()
        assert all(rows[33 + i, 1] == 2 * n + 26 for i, n in LONG_AT.items())
        for i in LONG_AT:
            r, rows = _check(ctx, oracle_lib, _dense_longid_file(i), "fastq", f"dense long ids flip at {i}")
            _tile_pass(r, f"flip at {i}")
            assert (len(rows), r.err) == (33 + i, ID_MISMATCH), (i, len(rows), r.err)


# ---- 4. records per tile --------------------------------------------------------------------------
DENSITY = [260, 256, 252, 136, 132, 131, 128, 124, 68, 66, 64, 60]
DENSE_TILES = 130


@pytest.mark.parametrize("B", DENSITY)
def test_fastq_records_per_tile_gpu(oracle_lib, B):
    """Uniform B-byte records over two whole placement groups, tile-aligned and behind a first
    record 1, 2, 3, 17 and 100 bytes longer.  260 / 256 / 252: 63 / 64 / 65 records per tile -- the
    64-entry line holds 63 starts and the last end, the 64th record's end is overflow entry 0.
    136 / 132 / 131: a group's entries fit PLACE_ECAP exactly (16 chunks per tile); 128 / 124: one
    chunk more per tile, so k_fq_place places tile by tile from global memory.  68 / 66: the most a
    fast tile holds; 64: 256 records and 1024 '\\n' per tile, past SNLCAP - NLHALO, and 60: every
    whole tile goes to k_fixup."""
    with _fresh() as ctx:
        for extra in (0, 1, 2, 3, 17, 100):
            data = gen.fq_uniform(B, DENSE_TILES * TILE + 4000, extra)  # (a last tile with a visible phase)
            nt = -(-len(data) // TILE)
            for fmt in ("fastq", "auto"):
                what = f"density B={B} extra={extra} fmt={fmt}"
                r, rows = _check(ctx, oracle_lib, data, fmt, what)
                _tile_pass(r, what)
                fixups, fix_tiles = _expect_fix(data, rows)
                assert (r.fixups, r.fix_tiles) == (fixups, fix_tiles), (what, r.fixups, r.fix_tiles, fixups, fix_tiles)
            if B >= 66:
                assert (fixups, fix_tiles) == (1, 0), (B, extra, fixups, fix_tiles)  # the file's end alone
            if B == 60:
                assert nt == DENSE_TILES + 1 and fix_tiles == nt - 1  # (the last, partial tile holds few enough lines)
            if B == 64:  # (behind a first record 100 bytes longer, tile 0 has 1017 '\n': fast, 255 records)
                assert fix_tiles == nt - (2 if extra == 100 else 1), (extra, fix_tiles)
            E = _place_entries(rows, nt)[:2]
            if B in (136, 132, 131):
                assert (E == PLACE_ECAP).all(), (B, extra, E)
            if B in (128, 124):
                assert (E > PLACE_ECAP).all(), (B, extra, E)
            if B >= 252:
                per = np.bincount(_owner(rows))[1:-1]
                assert {260: 63, 256: 64, 252: 65}[B] in set(per), (B, extra, sorted(set(per)))


def test_fastq_place_fallback_mixed_gpu(oracle_lib):
    """Placement groups of 128-byte records (the tile-by-tile fallback) next to groups of 512-byte
    records (the staged path): neighbouring k_fq_place workgroups take different branches."""
    dense = gen.fq_uniform(128, 64 * TILE)
    sparse = gen.fq_fill(64 * TILE)
    data = dense + sparse + dense + sparse[:TILE]
    assert len(dense) == 64 * TILE and len(data) == 193 * TILE
    with _fresh() as ctx:
        for fmt in ("fastq", "auto"):
            r, rows = _check(ctx, oracle_lib, data, fmt, f"mixed groups fmt={fmt}")
            _tile_pass(r, "mixed groups")
            assert (r.fixups, r.fix_tiles) == (1, 0), (r.fixups, r.fix_tiles)  # the file's end alone
        E = _place_entries(rows, len(data) // TILE)
        assert E[0] > PLACE_ECAP and E[1] <= PLACE_ECAP and E[2] > PLACE_ECAP and E[3] <= PLACE_ECAP, E


# ---- 5. deferred records per tile and the fix-up queue --------------------------------------------
def _padded_file(per_tile, ntiles=64):
    """ntiles whole tiles of 512-byte records; per_tile[t] of tile t's 32 records have a
    space-padded sequence line (valid to Go, which trims it; never certified by the tile pass)."""
    pad = gen.fq_rec(7, 249, pad=b" ")
    assert len(pad) == 512
    tiles = []
    for t in range(ntiles):
        plain = gen.fq_fill(TILE)
        assert len(plain) == TILE
        m = per_tile.get(t, 0)
        tiles.append(plain[:512 * (32 - m)] + pad * m if m else plain)
    return b"".join(tiles)


def test_fastq_max_defer_gpu(oracle_lib):
    """A tile with exactly 15, 16 (MAX_DEFER) and 17 records it cannot certify: 15 and 16 are queued
    one by one, the 17th turns the tile into one whole-tile item.  (One item more each: the file's
    end, in the last tile.)"""
    for m, want in ((15, (15 + 1, 0)), (16, (16 + 1, 0)), (17, (1 + 1, 1))):
        for t in (5, 31):
            with _fresh() as ctx:
                what = f"defer m={m} tile={t}"
                r, _ = _check(ctx, oracle_lib, _padded_file({t: m}), "fastq", what)
                _tile_pass(r, what)
                assert (r.fixups, r.fix_tiles) == want, (what, r.fixups, r.fix_tiles)


def test_fastq_fix_queue_capacity_gpu(oracle_lib):
    """The k_fixup queue of a context's first build holds _fixcap(ntiles) items: exactly that many
    (deferred records, at most MAX_DEFER per tile, and the file's end) are served by k_fixup, one
    more overflows the queue and the build is re-run two-pass.  Both tables are the oracle's."""
    cap = _fixcap(64)
    for extra, rerun in ((0, False), (1, True)):
        per, left = {}, cap - 1 + extra
        for t in range(3, 64, 2):
            per[t] = min(MAX_DEFER, left)
            left -= per[t]
        assert left == 0 and sum(per.values()) + 1 == cap + extra
        data = _padded_file(per)
        assert len(data) == 64 * TILE
        with _fresh() as ctx:
            r, _ = _check(ctx, oracle_lib, data, "fastq", f"queue cap={cap} items={cap + extra}")
            if rerun:
                assert r.reruns >= 1 and r.path == 2, (r.reruns, r.path)
            else:
                _tile_pass(r, "queue at capacity")
                assert (r.fixups, r.fix_tiles) == (cap, 0), (r.fixups, r.fix_tiles)


# ---- 6. every tile misreads its phase -------------------------------------------------------------
def _misread_file(extra, ntiles=70, bad_at=None):
    """128-byte records '@id / +ACG / +id / @III': after a quality line ('@') come an ID line and a
    line that starts with '+', and the ID and plus lines are equally long, so the phase read off a
    tile that does not start inside a quality line is early.  The first record is extra bytes
    longer; 128 divides TILE, so every tile starts at the same offset of a record.  bad_at: that
    record's quality line is one byte too long."""
    assert extra % 2 == 0

    def rec(i, more=0, qmore=0):
        rid = gen.fq_id(57, i)
        return b"@" + rid + b"\n+ACG" + b"A" * more + b"\n+" + rid + b"\n@III" + b"I" * (more + qmore) + b"\n"
    recs = [rec(i) for i in range(ntiles * TILE // 128)]
    assert all(len(x) == 128 for x in recs)
    recs[0] = rec(0, extra // 2)
    if bad_at is not None:
        recs[bad_at] = rec(bad_at, 0, 1)
    return b"".join(recs)


@pytest.mark.parametrize("extra", [0, 8, 34, 60, 100])
def test_fastq_phase_misread_gpu(oracle_lib, extra):
    """Every tile but the first (whose phase is known) reads its phase one line early and goes to
    k_fixup whole; the queue holds them all, so there is no re-run.  (Built as FASTQ: format
    detection rejects a sequence line that starts with '+'.)"""
    data = _misread_file(extra)
    nt = -(-len(data) // TILE)
    assert nt >= 70 and extra % 128 not in range(1, 5)  # no tile starts inside a quality line
    with _fresh() as ctx:
        what = f"misread extra={extra}"
        r, rows = _check(ctx, oracle_lib, data, "fastq", what)
        _tile_pass(r, what)
        assert r.err is None and len(rows) == 70 * TILE // 128
        assert (r.fixups, r.fix_tiles) == (nt - 1, nt - 1), (what, r.fixups, r.fix_tiles, nt)
        bad = _misread_file(extra, bad_at=4500)
        r, rows = _check(ctx, oracle_lib, bad, "fastq", what + " bad record 4500")
        _tile_pass(r, what)
        assert len(rows) == 4500 and r.err is not None and r.fix_tiles > 0, (len(rows), r.err, r.fix_tiles)


# ---- 7. the file end ------------------------------------------------------------------------------
def test_fastq_file_end_gpu(oracle_lib):
    """A file whose last record (CRLF, the ID on the plus line) lies wholly in the last tile, or
    across the seam into it, cut at every byte of that record; and whole files of 2 TILE + d bytes,
    d = -17 .. +17, with and without their last line end: the last tile's zero fill and the tail
    dword of a length that is no multiple of four."""
    last = gen.fq_rec(9, 17, eol=b"\r\n", plus_id=True, tag=3)
    with _fresh() as ctx:
        for head in (TILE + 5000, TILE - 30):
            base = gen.fq_fill(head) + last
            for cut in range(len(last) + 1):
                what = f"file end head={head} cut={cut}"
                r, _ = _check(ctx, oracle_lib, base[:len(base) - cut], "fastq", what)
                _tile_pass(r, what)
        for d in range(-17, 18):
            data = gen.fq_fill(2 * TILE + d - len(last)) + last
            assert len(data) == 2 * TILE + d
            for drop in (0, 1, 2):
                what = f"file end total=2*TILE{d:+d} drop={drop}"
                r, _ = _check(ctx, oracle_lib, data[:len(data) - drop], "fastq", what)
                _tile_pass(r, what)
                assert r.err is None, (what, r.err)


# ---- 8. the same corpora through the download filters and the slabs --------------------------------
def _selection():
    """A thinned selection of the corpora above: each seam with each mark at d = 0, each long-ID
    length once, dense tiles around the line / overflow, PLACE_ECAP and fast-tile edges, misread
    phases."""
    out = []
    for i, (name, k) in enumerate(sorted(SEAMS.items())):
        for mark in range(5):
            eol, plus_id, qual_at = THIN[(i + mark) % 2]
            lines = gen.fq_lines(11, 40, eol=eol, plus_id=plus_id, qual_at=qual_at, tag=k)
            out.append((f"seam {name} mark={mark}", _seam_file(k, mark, 0, lines)))
    for j, nid in enumerate(IDLENS):
        out.append((f"long id {nid}", _longid_file(nid, j % 4, (b"\n", b"\r\n")[j % 2])))
    out.append(("dense long ids", _dense_longid_file()))
    for B in (256, 128, 66):
        out.append((f"density {B}", gen.fq_uniform(B, DENSE_TILES * TILE, 3)))
    out.append(("misread", _misread_file(34)))
    return out


@pytest.fixture(scope="module")
def selection():
    return _selection()


def _filter_check(ctx, oracle_lib, data, name, what):
    r = ctx.filter_host(name, data)
    out, n, err = oracle_lib.filter_fastq(data, name)
    assert r.status in (0, 1), (what, r.status, r.err)
    assert (r.count, r.err) == (n, err), (what, r.count, r.err, n, err)
    assert r.gathered == out, what


@pytest.mark.parametrize("name", ["fq2fa", "anonymize"])
def test_fastq_tiles_filters_gpu(gpu_ctx, oracle_lib, selection, name):
    """The filters' spans come from the tile pass's line ends (k_fq_tiles<true> + k_fq_spans_place,
    u16 with the '\\r' bit, the same line / overflow entries): byte-exact on the selection."""
    for what, data in selection:
        _filter_check(gpu_ctx, oracle_lib, data, name, f"{name}: {what}")


def test_fastq_tiles_filters_rescan_gpu(gpu_ctx, oracle_lib, selection, monkeypatch):
    """The other span source (SHOCKIDX_FILTER_RESCAN: every record's lines re-read by k_fq_spans)
    is byte-exact on the same selection."""
    monkeypatch.setenv("SHOCKIDX_FILTER_RESCAN", "1")
    for what, data in selection:
        for name in ("fq2fa", "anonymize"):
            _filter_check(gpu_ctx, oracle_lib, data, name, f"rescan {name}: {what}")


def test_fastq_tiles_slabs_gpu(gpu_ctx, oracle_lib, selection, monkeypatch):
    """Three slabs with a cut on each of the probe's four line starts, the line start on a tile seam
    or 16 bytes past it (slab cuts are 16-byte aligned): a slab starts at every line phase next to a
    seam.  The rest of the selection runs over three even slabs."""
    from shock_amd import dist
    from test_gpu_slabs import _cmp
    plan = dist.plan_slabs
    for name, k in sorted(SEAMS.items()):
        for eol, plus_id, qual_at in THIN:
            lines = gen.fq_lines(11, 40, eol=eol, plus_id=plus_id, qual_at=qual_at, tag=k)
            for line in range(4):
                for off in (0, 16):
                    # line 0 starts at the '@'; line i at the byte after the previous line's '\n'
                    data = _seam_file(k, line, off - (1 if line else 0), lines)
                    cut = k * TILE + off
                    assert data[cut:cut + len(lines[line])] == lines[line]
                    cut2 = min(len(data), cut + TILE + 160)
                    monkeypatch.setattr(dist, "plan_slabs", lambda size, world, c=(cut, cut2): [(0, c[0]), c, (c[1], size)])
                    _cmp(gpu_ctx, oracle_lib, data, "fastq", 3)
    monkeypatch.setattr(dist, "plan_slabs", plan)
    for what, data in selection:
        if what.startswith("seam"):
            continue
        _cmp(gpu_ctx, oracle_lib, data, "fastq", 3)
