"""Column index (shockidx_column_device / _fd, CreateColumnIndex) against tests/colref.py, the
line-by-line restatement of index/column.go:33-130.  Every case runs through the default build
and through SHOCKIDX_COLUMN_MODE=two (the general build); both must give colref's status, count
and rows, and so agree with each other.

Cases: the known answers; sample1.sam at columns 1-12; lines, tabs and keys at and across the
16 KiB tile seams; keys and lines longer than a tile; runs of blank lines longer than two tiles;
CRLF; terminated / unterminated last lines; empty, single-group and all-distinct files; tiles
denser than any per-tile capacity; seeded random tables (one of 8 MiB); the missing-column error
(both of the reference's outcomes, error and panic); row capacity; CreateColumnIndex's file
protocol."""
import json
import os

import numpy as np
import pytest

import colref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "column", "kats.json")))
SAM = open(os.path.join(ROOT, "tests", "golden", "fixtures", "sample1.sam"), "rb").read()


def _pad(nbytes, key=b"p"):
    """Lines of one group (key, tab, filler) of exactly nbytes bytes in all (nbytes >= 4)."""
    out = bytearray()
    while nbytes - len(out) >= 204:
        out += key + b"\t" + b"f" * 97 + b"\n"
    rest = nbytes - len(out)
    assert rest >= len(key) + 2
    out += key + b"\t" + b"f" * (rest - len(key) - 2) + b"\n"
    return bytes(out)


def _table(seed, size, ncols=None):
    """A tab-separated table of exactly `size` bytes: every column in runs of 1-40 equal keys."""
    rng = np.random.default_rng(seed)
    ncols = ncols or int(rng.integers(3, 8))
    left = [0] * ncols
    cur = [b""] * ncols
    out = bytearray()
    while True:
        for j in range(ncols):
            if left[j] == 0:
                left[j] = int(rng.integers(1, 41))
                cur[j] = bytes(rng.integers(97, 123, int(rng.integers(1, 13)), dtype=np.uint8))
            left[j] -= 1
        line = b"\t".join(cur) + b"\n"
        if len(out) + len(line) + 2 * ncols + 2 > size:
            break
        out += line
    rest = size - len(out)  # a last line that fills the size exactly
    out += b"\t".join([b"z"] * (ncols - 1) + [b"z" * (rest - 2 * (ncols - 1) - 1)]) + b"\n"
    assert len(out) == size
    return bytes(out), ncols


def _cases():
    for i, k in enumerate(KATS):
        if "data" in k:
            yield f"kat{i:02d}", k["data"].encode("latin-1"), k["column"]
    for c in range(1, 13):
        yield f"sam_c{c}", SAM, c
    # ---- seams
    d = _pad(TILE) + b"p\ty\nm\tz\nm\tz\n"
    yield "seam_line_start_c1", d, 1
    yield "seam_line_start_c2", d, 2
    d = _pad(TILE - 2) + b"a\tv\na\tv\nb\tv\n" + _pad(TILE - 1, b"b") + b"c\tv\n"
    yield "seam_tab_last_byte_c1", d, 1
    yield "seam_tab_last_byte_c2", d, 2
    d = _pad(TILE - 5) + b"abcdefghij\tv\nabcdefghij\tw\nabcdefghiJ\tw\n" + _pad(TILE - 20, b"abcdefghiJ") + \
        b"u\tlonglonglonglonglongvalue\nu\tlonglonglonglonglongvalue\nu\tlonglonglonglonglongvalu3\n"
    yield "seam_key_straddles_c1", d, 1
    yield "seam_key_straddles_c2", d, 2
    big = b"x" * 40959
    yield "long_tabfree_lines", (big + b"\n") * 2 + big[:-1] + b"y\n" + big[:-1] + b"y\n" + (big + b"\n") + b"q\n", 1
    far = b"a\tb\tc\t" + b"d" * (TILE + 100) + b"\t"
    yield "key_far_from_line_start", (far + b"KEY\tz\n") * 2 + far + b"KEX\tz\n" + far + b"KEX\ty\n" + b"a\tb\tc\td\tKEX\n", 5
    wide = b"k\t" + b"w" * (5 * 1024) + b"\n"
    yield "wide_key_c2", wide * 3 + b"k\t" + b"w" * (5 * 1024 - 1) + b"v\n" + wide + b"k\t" + b"w" * 5000 + b"\n", 2
    # ---- blank lines
    gap = b"\n" * (2 * TILE + 50)
    yield "blank_run_equal_keys", b"k\t1\n" + gap + b"k\t2\n", 1
    yield "blank_run_different_keys", b"k\t1\n" + gap + b"j\t2\nj\t3\n" + gap + b"i\t4\n", 1
    yield "leading_blanks_then_key", b"\n" * 5 + b"k\t1\nk\t2\nj\t3\n", 1
    yield "leading_blanks_then_empty_key", b"\n" * 5 + b"\t1\n\t2\nj\t3\n", 1
    yield "leading_blank_tile_then_key", b"\n" * (TILE + 3) + b"k\t1\nk\t2\n", 1
    yield "line0_starts_with_tab", b"\ta\n\ta\nb\tc\nb\td\n", 1
    # ---- endings
    crlf = b"".join(b"k%d\tv%d\r\n" % (i // 7, i // 3) for i in range(3000))
    yield "crlf_c1", crlf, 1
    yield "crlf_c2", crlf, 2
    yield "last_column_terminated", b"a\tv\nb\tv\nc\tv\n", 2
    yield "last_column_unterminated", b"a\tv\nb\tv\nc\tv", 2
    yield "one_byte_last_line", b"a\t1\nb\t2\nx", 1
    yield "ends_in_two_newlines", b"a\t1\nb\t2\n\n", 1
    # ---- degenerate
    yield "empty", b"", 1
    yield "single_group_5_tiles", _pad(5 * TILE + 77, b"same"), 1
    yield "every_line_own_group", b"".join(b"k%d\tv\n" % i for i in range(6000)), 1
    # ---- dense
    rng = np.random.default_rng(5)
    dense = b"".join((b"a\n", b"bb\n")[int(x)] for x in rng.integers(0, 2, 4 * TILE // 2))[:4 * TILE + 1234]
    yield "dense_short_lines", dense + b"\n", 1
    mixed = b"".join(b"a\n" if x < 6 else (b"bb\n" if x < 9 else b"cc\t" + b"m" * 2996 + b"\n")
                     for x in rng.integers(0, 10, 800))[:6 * TILE + 321]
    yield "dense_mixed_with_3000", mixed, 1
    # ---- random tables
    for seed in (1, 2, 3):
        d, nc = _table(seed, 8 * TILE + 999)
        for c in sorted({1, 2, nc}):
            yield f"random_s{seed}_c{c}", d, c
    d, nc = _table(11, 8 << 20, 5)
    yield "random_8mib_c1", d, 1
    yield "random_8mib_c5", d, 5
    # ---- errors
    lines = [b"k%d\ta\tb\n" % (i // 9) for i in range(5000)]
    good = b"".join(lines)  # > 2 tiles
    short = b"k\ta\n"
    yield "err_short_line_third_tile", good + short + b"".join(lines[:40]), 3  # t + 2 == c: the reference panics
    yield "err_short_line_reference_errors", good + b"kk\n" + b"".join(lines[:40]), 3  # t + 1 < c - 1: its error
    yield "err_two_bad_lines", b"".join(lines[:100]) + short + good + b"kk\n", 3
    yield "blank_line_is_no_error", b"".join(lines[:100]) + b"\n" + b"".join(lines[100:300]) + b"x", 3


CASES = {name: (data, c) for name, data, c in _cases()}
_REF = {}


def _ref(name):
    if name not in _REF:
        data, c = CASES[name]
        _REF[name] = colref.expected(data, c)
    return _REF[name]


def _check(r, want, what):
    from shock_amd import _lib as L
    if want[0] == "err":
        assert r.status == L.EFORMAT and r.err == colref.MESSAGE and r.count == 0, (what, r.status, r.err, r.count)
        return
    exp = np.array(want[1], dtype=np.uint64).reshape(-1, 2)
    assert r.status == L.OK and r.err is None, (what, r.status, r.err)
    assert r.fmt == "line"
    assert r.count == len(exp), (what, r.count, len(exp))
    got = r.rows if r.rows is not None else np.zeros((0, 2), np.uint64)
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0][:5]
        raise AssertionError(f"{what}: rows {bad.tolist()}: gpu {got[bad].tolist()} colref {exp[bad].tolist()}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_column_vs_colref(gpu_ctx, name, monkeypatch):
    data, c = CASES[name]
    want = _ref(name)
    monkeypatch.delenv("SHOCKIDX_COLUMN_MODE", raising=False)
    a = gpu_ctx.column_host(data, c)
    _check(a, want, f"{name} (default)")
    monkeypatch.setenv("SHOCKIDX_COLUMN_MODE", "two")
    b = gpu_ctx.column_host(data, c)
    _check(b, want, f"{name} (two)")
    assert a.path == 1 and b.path == 2
    assert a.status == b.status and a.count == b.count


def test_case_statuses_are_what_the_names_say():
    """The error cases hit both of the reference's outcomes; the others are tables."""
    data, c = CASES["err_short_line_third_tile"]
    assert colref.column_index(data, c) == ("panic",) and len(data) > 2 * TILE
    data, c = CASES["err_short_line_reference_errors"]
    assert colref.column_index(data, c) == ("err",)
    data, c = CASES["err_two_bad_lines"]
    assert colref.column_index(data, c) == ("panic",)  # the earlier bad line decides
    for name in ("blank_line_is_no_error", "single_group_5_tiles", "dense_short_lines", "random_8mib_c5"):
        assert _ref(name)[0] == "ok"
    assert _ref("single_group_5_tiles")[1] == [] and len(_ref("random_8mib_c1")[1]) > 1000


def test_sam_golden_tables(gpu_ctx):
    for k in KATS:
        if "fixture" not in k:
            continue
        r = gpu_ctx.column_host(SAM, k["column"])
        want = ("ok", [tuple(x) for x in k["rows"]]) if k["status"] == "ok" else ("err",)
        _check(r, want, f"sample1.sam column {k['column']}")


def test_column_zero_is_einval(gpu_ctx):
    from shock_amd import _lib as L
    for c in (0, -3):
        r = gpu_ctx.column_host(b"a\tb\n", c)
        assert r.status == L.EINVAL and r.count == 0


@pytest.mark.parametrize("mode", ["default", "two"])
def test_row_capacity(gpu_ctx, mode, monkeypatch):
    from shock_amd import _lib as L
    if mode == "two":
        monkeypatch.setenv("SHOCKIDX_COLUMN_MODE", "two")
    else:
        monkeypatch.delenv("SHOCKIDX_COLUMN_MODE", raising=False)
    data, c = CASES["random_s1_c1"]
    want = np.array(_ref("random_s1_c1")[1], dtype=np.uint64)
    need = len(want)
    assert need > 8
    d_in = gpu_ctx.alloc(len(data) + 64)
    d_in.upload(data)
    d_rows = gpu_ctx.alloc(16 * need)
    try:
        r = gpu_ctx.column_device(d_in.ptr, len(data), c, d_rows.ptr, need - 1)
        assert r.status == L.ESPACE and r.count == need
        r = gpu_ctx.column_device(d_in.ptr, len(data), c, d_rows.ptr, need)
        assert r.status == L.OK and r.count == need
        assert np.array_equal(d_rows.rows(need), want)
    finally:
        d_in.free()
        d_rows.free()


def test_column_fd(gpu_ctx, tmp_path):
    for name in ("random_s2_c1", "single_group_5_tiles", "err_two_bad_lines", "empty"):
        data, c = CASES[name]
        p = tmp_path / "body"
        p.write_bytes(data)
        with open(p, "rb") as f:
            r = gpu_ctx.column_fd(f.fileno(), len(data), c)
        _check(r, _ref(name), f"{name} (fd)")


def test_create_column_index(gpu_ctx, tmp_path, monkeypatch):
    from shock_amd import indexer
    monkeypatch.setattr(indexer, "PATH_DATA", str(tmp_path / "data"))
    monkeypatch.setattr(indexer, "_ctx", gpu_ctx)
    tmpdir = tmp_path / "data" / "temp"
    for name in ("random_s3_c1", "single_group_5_tiles"):
        data, c = CASES[name]
        body = tmp_path / "body"
        body.write_bytes(data)
        out = tmp_path / f"{name}.idx"
        idx = indexer.NewColumnIndexer(open(body, "rb"))
        count, fmt, err = indexer.CreateColumnIndex(idx, c, str(out))
        idx.close()
        want = np.array(_ref(name)[1], dtype="<u8").reshape(-1, 2)
        assert (count, fmt, err) == (len(want), "array", None)
        assert out.read_bytes() == want.tobytes()
        assert list(tmpdir.iterdir()) == []
    data, c = CASES["err_short_line_third_tile"]
    body = tmp_path / "bad"
    body.write_bytes(data)
    out = tmp_path / "bad.idx"
    idx = indexer.NewColumnIndexer(open(body, "rb"))
    count, fmt, err = indexer.CreateColumnIndex(idx, c, str(out))
    idx.close()
    assert count == 0 and fmt == "array" and isinstance(err, indexer.ShockIndexError)
    assert err.msg == colref.MESSAGE
    assert not out.exists() and list(tmpdir.iterdir()) == []
