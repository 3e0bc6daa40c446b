"""The column index's slab walk over a file (shockidx_column_fd_walk), CreateColumnIndex's file
protocol over it (shockidx_column_create) and its bounded device footprint: a node that does not
fit the context's device cap is indexed through two slots sized to the cap, with the table of the
whole-node build."""
import numpy as np
import pytest

import colref
from test_gpu_column import CASES, _table

pytestmark = pytest.mark.gpu

MIB = 1 << 20
_DATA = {}


def _mib_table():
    """a seeded table of about 1 MiB (5 columns) and colref's answers for columns 1 and 5"""
    if not _DATA:
        d, nc = _table(23, MIB + 777, 5)
        _DATA["d"] = d
        for c in (1, nc):
            _DATA[c] = np.array(colref.expected(d, c)[1], dtype=np.uint64).reshape(-1, 2)
    return _DATA


def _file(tmp_path, data, name="body"):
    p = tmp_path / name
    p.write_bytes(data)
    return p


@pytest.mark.parametrize("c", [1, 5])
def test_fd_walk_table(gpu_ctx, tmp_path, c):
    from shock_amd import _lib as L
    t = _mib_table()
    data, want = t["d"], t[c]
    assert len(want) > 1000
    p = _file(tmp_path, data)
    with open(p, "rb") as f:
        r = gpu_ctx.column_fd_walk(f.fileno(), len(data), c, 32 << 10, 4 << 10)
    assert r.status == L.OK and r.path == 5 and r.fmt == "line" and r.reruns == 0
    assert r.count == len(want) and np.array_equal(r.rows, want)


@pytest.mark.parametrize("name", ["err_short_line_third_tile", "err_short_line_reference_errors", "err_two_bad_lines"])
def test_fd_walk_errors(gpu_ctx, tmp_path, name):
    from shock_amd import _lib as L
    data, c = CASES[name]
    p = _file(tmp_path, data)
    with open(p, "rb") as f:
        r = gpu_ctx.column_fd_walk(f.fileno(), len(data), c, 32 << 10, 4 << 10)
    assert r.status == L.EFORMAT and r.err == colref.MESSAGE and r.count == 0 and r.path == 5
    assert r.rows is None


def test_fd_walk_small_and_degenerate(gpu_ctx, tmp_path):
    """an empty file, a single group, slabs off the tile grid, a line that needs the retry rule, and
    a line no slot can hold"""
    from shock_amd import _lib as L
    for name, S, halo in (("empty", 32 << 10, 4096), ("single_group_5_tiles", 16 << 10, 16),
                          ("random_s1_c1", 3 * 16384 + 16, 4096), ("key_far_from_line_start", 16384, 4096),
                          ("straddle", 16384, 16)):
        data, c = CASES[name] if name != "straddle" else (b"p\tv\n" * 4093 + (b"K" * 40 + b"\tv\n") * 2 + b"r\tv\n", 1)
        p = _file(tmp_path, data, name)
        with open(p, "rb") as f:
            r = gpu_ctx.column_fd_walk(f.fileno(), len(data), c, S, halo)
        want = np.array(colref.expected(data, c)[1], dtype=np.uint64).reshape(-1, 2)
        assert r.status == L.OK and r.path == 5 and r.count == len(want), name
        assert np.array_equal(r.rows if r.rows is not None else np.zeros((0, 2), np.uint64), want), name
        # a 40-byte key from 12 bytes before the slab's end, a 16-byte halo: the slab is shortened once
        assert r.reruns == (1 if name == "straddle" else 0), name
    data, c = CASES["long_tabfree_lines"]
    p = _file(tmp_path, data, "long")
    with open(p, "rb") as f, pytest.raises(L.ShockIdxError) as e:
        gpu_ctx.column_fd_walk(f.fileno(), len(data), c, 16384, 4096)
    assert e.value.code == L.ENOMEM and "slot" in e.value.msg


def test_fd_walk_rows_past_one_pinned_chunk(gpu_ctx, tmp_path):
    """one slab with more rows than the pinned row buffer holds (64 MiB / 16 = 4 Mi rows): the row
    drain loops, numbers its second chunk from where the first ended and checks the table across
    the seam.  Two-byte lines with alternating keys: every line is a row (2 i, 2)."""
    from shock_amd import _lib as L
    lines = (4 << 20) + 1000
    data = b"a\nb\n" * (lines // 2)
    assert len(data) == 8390608
    p = _file(tmp_path, data)
    with open(p, "rb") as f:
        r = gpu_ctx.column_fd_walk(f.fileno(), len(data), 1, 16 << 20, 4096)  # (S is clipped to the file: one slab)
    # the rows outgrow the slab's first table (S / 32 + 4096) once
    assert r.status == L.OK and r.path == 5 and r.reruns == 1 and r.count == lines == 4195304
    want = np.array(colref.expected(data, 1)[1], dtype=np.uint64).reshape(-1, 2)
    closed = np.stack([2 * np.arange(lines, dtype=np.uint64), np.full(lines, 2, np.uint64)], axis=1)
    assert np.array_equal(want, closed)
    assert np.array_equal(r.rows, want)


def test_column_create_protocol(gpu_ctx, tmp_path):
    """a node that fits the budget takes the whole-node build (path 1); the .idx is colref's table"""
    from shock_amd import _lib as L
    t = _mib_table()
    tmpdir = tmp_path / "temp"
    tmpdir.mkdir()
    p = _file(tmp_path, t["d"])
    out = tmp_path / "t.idx"
    with open(p, "rb") as f:
        r = gpu_ctx.column_create(f.fileno(), len(t["d"]), 1, str(tmpdir), str(out))
    assert r.status == L.OK and r.path == 1 and r.count == len(t[1])
    assert out.read_bytes() == t[1].astype("<u8").tobytes() and list(tmpdir.iterdir()) == []


def _capped(cap):
    from shock_amd import Context
    ctx = Context(0)
    ctx.set_dev_cap(cap)
    return ctx


def _block_node(tmp_path, nbytes, last_line=b""):
    """a seeded 1 MiB block repeated, the last copy cut, to nbytes in all (+ last_line)"""
    block = _mib_table()["d"][:MIB]
    p = tmp_path / "node"
    with open(p, "wb") as f:
        left = nbytes
        while left:
            k = min(left, len(block))
            f.write(block[:k])
            left -= k
        f.write(last_line)
    return p, nbytes + len(last_line)


def test_column_create_through_the_walk(tmp_path):
    """a node over the cap: the rows reach the .idx slab by slab; byte-identical to colref's table"""
    from shock_amd import _lib as L
    cap = 32 * MIB
    p, n = _block_node(tmp_path, 16 * MIB + 4321)
    data = p.read_bytes()
    want = np.array(colref.expected(data, 1)[1], dtype="<u8").reshape(-1, 2)
    tmpdir = tmp_path / "temp"
    tmpdir.mkdir()
    out = tmp_path / "t.idx"
    ctx = _capped(cap)
    try:
        with open(p, "rb") as f:
            r = ctx.column_create(f.fileno(), n, 1, str(tmpdir), str(out))
        assert r.status == L.OK and r.path == 5 and r.count == len(want)
        assert out.read_bytes() == want.tobytes() and list(tmpdir.iterdir()) == []
        assert ctx.workspace_bytes() <= cap
    finally:
        ctx.close()


def test_column_create_single_group_and_late_error(tmp_path):
    """through the walk: one group over the whole node leaves a zero-byte file; a line without the
    column in the last slab, after rows were written, leaves no output and an empty temp dir"""
    from shock_amd import _lib as L
    cap = 32 * MIB
    tmpdir = tmp_path / "temp"
    tmpdir.mkdir()
    ctx = _capped(cap)
    try:
        line = b"same\t" + b"f" * 58 + b"\n"
        p = tmp_path / "one"
        p.write_bytes(line * (16 * MIB // len(line)))
        out = tmp_path / "one.idx"
        with open(p, "rb") as f:
            r = ctx.column_create(f.fileno(), p.stat().st_size, 1, str(tmpdir), str(out))
        assert r.status == L.OK and r.path == 5 and r.count == 0
        assert out.exists() and out.stat().st_size == 0 and list(tmpdir.iterdir()) == []
        p, n = _block_node(tmp_path, 16 * MIB, b"\nk\ta\n")  # the only lines without column 3 end the file
        out = tmp_path / "bad.idx"
        with open(p, "rb") as f:
            r = ctx.column_create(f.fileno(), n, 3, str(tmpdir), str(out))
        assert r.status == L.EFORMAT and r.err == colref.MESSAGE and r.count == 0 and r.path == 5
        assert not out.exists() and list(tmpdir.iterdir()) == []
    finally:
        ctx.close()


def test_bounded_footprint(tmp_path):
    from shock_amd import Context, _lib as L
    cap = 32 * MIB
    p, n = _block_node(tmp_path, 64 * MIB + 4321)
    small = _capped(cap)
    free = Context(0)
    try:
        with open(p, "rb") as f:
            a = small.column_fd(f.fileno(), n, 1)
            held = small.workspace_bytes()
            b = free.column_fd(f.fileno(), n, 1)
        assert a.status == L.OK and a.path == 5, (a.status, a.path)
        assert held <= cap, held
        assert b.status == L.OK and b.path == 1
        assert a.count == b.count and a.count > 50000 and np.array_equal(a.rows, b.rows)
        rows = a.rows
        assert rows[0, 0] == 0 and int(rows[-1, 0] + rows[-1, 1]) == n
        assert np.array_equal(rows[1:, 0], rows[:-1, 0] + rows[:-1, 1])
    finally:
        small.close()
        free.close()
