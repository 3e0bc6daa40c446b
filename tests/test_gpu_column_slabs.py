"""The column index's slab pass (shockidx_column_slab_device) against tests/colref.py: a file walked
slab by slab through tests/colslab.py must give the table of the whole build, whatever the slab
size, the halo and where the slab ends fall.

What a walk must end with is worked out from the bytes alone (_expected): colref's table or error,
unless a line the walk reaches first cannot be settled by any slot -- from the '\n' before it, a
slab and its halo do not reach its key's closing tab (or, for a key in the last field or a line with
too few fields, its end) -- which is the driver's "nomem" decision, never a short table.
"""
import numpy as np
import pytest

import colref
import colslab
import test_gpu_column as whole
from test_gpu_column import CASES, TILE

pytestmark = pytest.mark.gpu

BIG = ("random_8mib_c1", "random_8mib_c5")
REST = 1 << 40  # a halo of the rest of the file
CONFIGS = [(S, h) for S in (TILE, 2 * TILE, 3 * TILE, 3 * TILE + 16) for h in (16, 4096, REST)]


def _lines(data, c):
    """(start, settle_end, bad) per non-blank line: where its key closes (its c-th tab + 1, else its
    end) and whether it has fewer than c fields."""
    out = []
    pos = 0
    for buf, _eof in colref.read_lines(data):
        n = len(buf)
        if n > 1:
            tabs = [i for i, b in enumerate(buf) if b == 9][:c]
            bad = len(tabs) + 1 < c
            out.append((pos, pos + (tabs[c - 1] + 1 if len(tabs) == c else n), bad))
        pos += n
    return out


def _expected(data, c, S, halo, lines=None):
    size = len(data)
    for x, settle, bad in (lines if lines is not None else _lines(data, c)):
        reach = min(S + halo, size) if x == 0 else min(x - 1 + S + halo, size)
        if settle > reach:
            return ("nomem",)
        if bad:
            return ("err",)
    return colref.expected(data, c)


def _check(got, want, what):
    outcome, rows, log = got
    if want[0] != "ok":
        assert outcome == want[0], (what, outcome, log[-3:])
        if outcome == "err":
            assert rows == colref.MESSAGE
        return
    exp = np.array(want[1], dtype=np.uint64).reshape(-1, 2)
    assert outcome == "ok", (what, outcome, log[-3:])
    if not np.array_equal(rows, exp):
        k = min(len(rows), len(exp))
        bad = np.nonzero((rows[:k] != exp[:k]).any(axis=1))[0][:5]
        raise AssertionError(f"{what}: {len(rows)} rows, colref {len(exp)}; first differing {bad.tolist()}: "
                             f"gpu {rows[bad].tolist()} colref {exp[bad].tolist()}")


@pytest.mark.parametrize("name", sorted(n for n in CASES if n not in BIG))
def test_slab_sweep(gpu_ctx, name):
    data, c = CASES[name]
    lines = _lines(data, c)
    for S, halo in CONFIGS:
        want = _expected(data, c, S, halo, lines)
        if want[0] == "ok":
            assert want == whole._ref(name)
        _check(colslab.walk(gpu_ctx, data, c, S, halo), want, f"{name} S={S} halo={halo}")


@pytest.mark.parametrize("name", BIG)
def test_slab_sweep_8mib(gpu_ctx, name):
    data, c = CASES[name]
    got = colslab.walk(gpu_ctx, data, c, 64 * TILE, 4096)
    _check(got, whole._ref(name), name)
    assert len(got[2]) == 8  # eight slabs, none submitted twice


# ---- constructed seams, at 1-tile slabs ----------------------------------------------------------
def _two(lines, c):
    """lines of (key, other) with the key in column c of 2"""
    return b"".join((k + b"\t" + o if c == 1 else o + b"\t" + k) + b"\n" for k, o in lines)


def _seams():
    for c in (1, 2):
        tag = f"c{c}"
        grp = lambda k, m: [(k, b"v")] * m  # noqa: E731
        # a '\n' that is the slab's last byte, and so a line that starts exactly at a slab start
        head = _two(grp(b"p", TILE // 4 - 1), c)  # 4 bytes a line
        assert len(head) == TILE - 4
        d = head + _two([(b"p", b"v"), (b"q", b"v"), (b"q", b"v"), (b"r", b"v")], c)
        assert d[TILE - 1] == 10
        yield f"newline_last_byte_{tag}", d, c, None
        # a key straddling the slab end: inside the halo, and past it
        key = b"abcdefghijklmnopqrstuvwxyz0123456789ABCD"  # 40 bytes
        d = head[:-8] + _two([(key, b"v"), (key, b"v"), (key[:-1] + b"x", b"v"), (b"r", b"v")], c)
        at = d.index(key)
        assert at < TILE < at + len(key)
        yield f"key_straddles_{tag}", d, c, None
        # a tab as the last byte of a slab
        d = head[:-4] + _two([(b"pp", b"v"), (b"pp", b"v"), (b"q", b"v")], c) if c == 1 else \
            head[:-4] + _two([(b"p", b"vv"), (b"p", b"vv"), (b"q", b"vv")], c)
        assert d[TILE - 1] == 9, d[TILE - 4:TILE + 4]
        yield f"tab_last_byte_{tag}", d, c, None
        # blank lines over two whole slabs and more: the carry passes through
        gap = b"\n" * (2 * TILE + 50)
        yield f"blank_slabs_equal_keys_{tag}", _two([(b"k", b"1")], c) + gap + _two([(b"k", b"1"), (b"j", b"1")], c), c, None
        yield f"blank_slabs_different_keys_{tag}", _two([(b"k", b"1")], c) + gap + _two([(b"j", b"1")], c) + gap + _two([(b"i", b"1")], c), c, None
        yield f"leading_blank_slabs_then_key_{tag}", gap + _two([(b"k", b"1"), (b"k", b"1"), (b"j", b"1")], c), c, None
        if c == 1:
            yield "leading_blank_slabs_then_empty_key_c1", gap + b"\t1\n\t2\nj\t3\n", 1, None
        yield f"single_group_5_slabs_{tag}", _two(grp(b"same", 5 * TILE // 7 + 9), c), c, []
        yield f"every_line_own_group_{tag}", _two([(b"k%d" % i, b"v") for i in range(5000)], c), c, None
        yield f"crlf_{tag}", b"".join((b"k%d\tv\r\n" if c == 1 else b"v\tk%d\r\n") % (i // 7) for i in range(3000)), c, None
        yield f"unterminated_last_line_{tag}", _two(grp(b"a", 5000) + grp(b"b", 3), c)[:-1], c, None
        yield f"one_byte_last_line_{tag}", _two(grp(b"a", 4095) + [(b"b", b"v")], c) + b"x", c, None
        yield f"one_byte_last_line_own_slab_{tag}", _two(grp(b"a", 4095) + [(b"b", b"v")], c) + b"\n" * 12 + b"x", c, None


SEAMS = {name: (d, c, rows) for name, d, c, rows in _seams()}


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams(gpu_ctx, name):
    data, c, rows = SEAMS[name]
    want = colref.expected(data, c)
    assert want[0] == "ok" and (rows is None or want[1] == rows)
    from shock_amd import _lib as L
    for halo in (16, 4096, REST):
        assert _expected(data, c, TILE, halo) == want
        got = colslab.walk(gpu_ctx, data, c, TILE, halo)
        _check(got, want, f"{name} halo={halo}")
        if name.startswith("key_straddles") and halo == 16:
            more = [e for e in got[2] if e[2] == L.EMORE]
            # the key does not close in the 16 bytes past the slab: the slab gives the line up
            assert more and more[0][0] == 0 and data[more[0][3] - 1] == 10 and more[0][3] < TILE
        else:
            assert all(e[2] in (L.OK, L.ESPACE) for e in got[2]), got[2]  # (ESPACE: the driver's rows grow)


# ---- retry and error behaviour -------------------------------------------------------------------
def test_line_longer_than_a_slot_is_nomem(gpu_ctx):
    S, halo = TILE, 4096
    data = b"a\t1\n" * 100 + b"b\t" + b"x" * (16 + S + halo + 1) + b"\n" + b"c\t1\n"
    for c in (1, 2):
        want = _expected(data, c, S, halo)
        # column 1's key closes at the first tab; the last column's only at the line's end
        assert want == (colref.expected(data, c) if c == 1 else ("nomem",))
        _check(colslab.walk(gpu_ctx, data, c, S, halo), want, f"long line c={c}")


@pytest.mark.parametrize("tail", [b"m\tv\nm\tv\nn\tv\n", b""])
def test_key_longer_than_the_carry(gpu_ctx, tail):
    """A slab's last non-blank line with a 70 KiB key: the carry cannot hold it, the slab gives the
    line up (EMORE) and the next slab owns it -- where other lines follow it, or no slab does."""
    from shock_amd import _lib as L
    S, halo = 8 * TILE, 80 << 10
    head = b"a\tx\n" * 25000 + b"b\tx\n"
    big = b"K" * (70 << 10)
    data = head + big + b"\tv\n" + tail
    x = len(head)
    assert x < S < x + len(big) and x + len(big) < S + halo and len(big) > L.COLUMN_KEYCAP
    got = colslab.walk(gpu_ctx, data, 1, S, halo)
    _check(got, colref.expected(data, 1), "70 KiB key")
    assert got[2] == [(0, S, L.EMORE, x), (0, x - 1, L.OK, 1), (x - 1, len(data) - x + 1, L.OK, 2 + (2 if tail else 0))]


def test_keys_longer_than_the_carry_in_a_row(gpu_ctx):
    """Three such lines in a row with slabs that hold fewer than two of them: shortened, a slab's
    last non-blank line is one of them again, now at its head -- no slot can carry that key on."""
    from shock_amd import _lib as L
    S, halo = 8 * TILE, 80 << 10
    big = b"K" * (70 << 10)
    data = b"a\tx\n" * 25001 + (big + b"\tv\n") * 3 + b"m\tv\n"
    outcome, _, log = colslab.walk(gpu_ctx, data, 1, S, halo)
    assert outcome == "nomem" and log[-1][2] == L.EMORE and log[-1][3] - 1 == log[-1][0]
    # with 16-tile slabs the first one is shortened until it ends before them, and the rest is the file's last slab
    _check(colslab.walk(gpu_ctx, data, 1, 16 * TILE, halo), colref.expected(data, 1), "three 70 KiB keys")


def _slab(L, ptr, lo, n, end, size):
    return L.Slab(d_data=ptr, n=n, end=end, front=lo, base=lo, is_first=int(lo == 0), is_last=int(lo + n == size),
                  seq=0, reserved=0)


def test_espace_leaves_the_carry_untouched(gpu_ctx):
    from shock_amd import _lib as L
    data = b"".join(b"k%d\tv\n" % (i // 3) for i in range(9000))
    size = len(data)
    want = np.array(colref.expected(data, 1)[1], dtype=np.uint64).reshape(-1, 2)
    S = 2 * TILE
    assert size > S + TILE
    d_in = gpu_ctx.alloc(size + 64)
    d_in.upload(data)
    carry = gpu_ctx.column_carry()
    d_rows = gpu_ctx.alloc(16 * 4096)
    try:
        r0 = gpu_ctx.column_slab(_slab(L, d_in.ptr, 0, S, S + 64, size), size, 1, carry.ptr, d_rows.ptr, 4096)
        assert r0.status == L.OK and r0.count > 8
        rows = [d_rows.rows(r0.count)]
        s1 = _slab(L, d_in.ptr + S, S, size - S, size - S, size)
        probe = gpu_ctx.column_slab(s1, size, 1, carry.ptr, d_rows.ptr, 0)
        assert probe.status == L.ESPACE
        need = probe.count
        assert r0.count + need == len(want)
        r = gpu_ctx.column_slab(s1, size, 1, carry.ptr, d_rows.ptr, need - 1)
        assert r.status == L.ESPACE and r.count == need
        r = gpu_ctx.column_slab(s1, size, 1, carry.ptr, d_rows.ptr, need)
        assert r.status == L.OK and r.count == need and r.path == 5
        rows.append(d_rows.rows(need))
        assert np.array_equal(np.concatenate(rows), want)
    finally:
        d_in.free()
        carry.free()
        d_rows.free()


@pytest.mark.parametrize("bad,ref", [(b"k\ta\n", "panic"), (b"kk\n", "err")])
def test_missing_column_in_the_third_slab(gpu_ctx, bad, ref):
    """after two slabs that produced rows; both of the reference's outcomes are EFORMAT, count 0"""
    from shock_amd import _lib as L
    lines = [b"k\ta\tv%d\n" % (i // 9) for i in range(6000)]
    good = b""
    for ln in lines:
        good += ln
        if len(good) > 2 * TILE + 100:
            break
    data = good + bad + b"".join(lines[:40])
    assert 2 * TILE < len(good) < 3 * TILE and colref.column_index(data, 3) == (ref,)
    outcome, msg, log = colslab.walk(gpu_ctx, data, 3, TILE, 4096)
    assert outcome == "err" and msg == colref.MESSAGE
    assert [e[2] for e in log] == [L.OK, L.OK, L.EFORMAT] and log[0][3] > 100 and log[1][3] > 100  # rows came first


@pytest.mark.parametrize("bad,ref", [(b"k\ta\n", "panic"), (b"kk\n", "err")])
def test_missing_column_line_spans_a_slab_end(gpu_ctx, bad, ref):
    line = b"k\ta\tb\n"
    k = (TILE - 2) // len(line) - 1
    data = line * k + b"j\ta\t" + b"b" * (TILE - 2 - len(line) * k - 5) + b"\n"
    assert len(data) == TILE - 2  # the bad line starts two bytes before the slab's end
    data += bad + line * 10
    assert colref.column_index(data, 3) == (ref,)
    for halo in (16, 4096):
        outcome, msg, log = colslab.walk(gpu_ctx, data, 3, TILE, halo)
        assert outcome == "err" and msg == colref.MESSAGE and len(log) == 1


def test_invalid_slabs_are_einval(gpu_ctx):
    from shock_amd import _lib as L
    d_in = gpu_ctx.alloc(4096)
    carry = gpu_ctx.column_carry()
    try:
        ok = dict(d_data=d_in.ptr, n=100, end=100, front=0, base=0, is_first=1, is_last=1, seq=0, reserved=0)
        for change in (dict(is_first=0), dict(is_last=0), dict(end=99), dict(end=101), dict(d_data=d_in.ptr + 8),
                       dict(base=64, is_first=0, front=8)):
            s = L.Slab(**{**ok, **change})
            size = 100 + s.base
            assert gpu_ctx.column_slab(s, size, 1, carry.ptr, 0, 0).status == L.EINVAL, change
        assert gpu_ctx.column_slab(L.Slab(**ok), 100, 0, carry.ptr, 0, 0).status == L.EINVAL
    finally:
        d_in.free()
        carry.free()
