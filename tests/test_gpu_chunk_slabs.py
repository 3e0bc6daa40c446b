"""GPU: the chunkrecord index in slabs (shockidx_chunkrecord_slab_device, shockidx_chunkrecord_fd_walk
and shockidx_chunkrecord_fd under a device cap) against the C oracle and against
shockidx_chunkrecord_device on the whole buffer.  The file is uploaded once; a slab is a sub-window
[lo, hi) of that buffer given as base (16-byte aligned, the first such offset in the window), front =
base - lo and end = hi - base.  Bar: the slabs' rows concatenated, the per-slab counts' sum and the
final carry's count all equal the oracle's, whichever way the file is cut, in both chunk modes."""
import os
import random
import zlib

import numpy as np
import pytest

from test_chunk_slab_model import (CHUNKS, FRONTS, STRIDES, cut_views, make, stride_views, window_of_row)
from test_oracle_chunk import WIN, fastq_records

pytestmark = pytest.mark.gpu

EINVAL, ESPACE, EFORMAT = -1, -6, 1


@pytest.fixture(params=["spec", "serial"])
def chunk_mode(request, monkeypatch):
    if request.param == "serial":
        monkeypatch.setenv("SHOCKIDX_CHUNK_MODE", "serial")
    else:
        monkeypatch.delenv("SHOCKIDX_CHUNK_MODE", raising=False)
    return request.param


class Node:
    """A file in HBM with its expectations (uploaded once, shared by every cut of a test)."""

    def __init__(self, ctx, oracle_lib, data, fmt, chunk):
        self.ctx, self.data, self.n, self.fmt, self.chunk = ctx, data, len(data), fmt, chunk
        self.exp, err = oracle_lib.chunkrecord(data, fmt, chunk or oracle_lib.CHUNK_SIZE)
        assert err is None
        self.buf = ctx.alloc(self.n + 64)
        if self.n:
            self.buf.upload(data)
        self.cap = ctx.chunkrecord_capacity(self.n, chunk)
        self.rows = ctx.alloc(16 * self.cap)
        self.carry = ctx.chunkrecord_carry()
        r = ctx.chunkrecord_buffer(self.buf, self.n, self.rows, fmt=fmt, chunk=chunk)  # the whole-node build agrees
        assert r.ok and r.count == len(self.exp) and np.array_equal(self.rows.rows(r.count), self.exp)

    def slab(self, lo, hi, fmt="carry", rows=None, first=None):
        base = (lo + 15) & ~15
        assert base <= hi, (lo, hi)
        return self.ctx.chunkrecord_slab(self.buf, base, base - lo, hi - base, self.n, self.carry, rows or self.rows,
                                         fmt=self.fmt if fmt == "carry" else fmt, chunk=self.chunk, first=first)

    def carry_state(self):
        w = self.carry.download().view(np.uint64)
        h = w[8 + 8 * int(w[0] & 1):]
        return {"curr": int(h[0]), "off": int(h[1]), "count": int(h[2]), "fmt": int(h[3]), "done": int(h[4])}

    def walk(self, views, tag=""):
        got, per = [], []
        for i, (lo, hi) in enumerate(views):
            r = self.slab(lo, hi, first=i == 0)  # (a later window may start at 0 too)
            assert r.ok and r.path == 6, (tag, lo, hi, r)
            per.append(r.count)
            if r.count:
                got.append(self.rows.rows(r.count))
        rows = np.concatenate(got) if got else np.zeros((0, 2), np.uint64)
        st = self.carry_state()
        assert sum(per) == len(self.exp) == st["count"] and st["done"] == 1, (tag, sum(per), len(self.exp), st)
        assert np.array_equal(rows, self.exp), (tag, rows[:4], self.exp[:4])
        return per

    def free(self):
        for b in (self.buf, self.rows, self.carry):
            b.free()


@pytest.mark.parametrize("fmt,variant", [("fastq", "plain"), ("fastq", "crlf"), ("fastq", "atqual"), ("fasta", "plain"),
                                         ("fasta", "crlf")])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_slab_sweep_of_cuts(gpu_ctx, oracle_lib, fmt, variant, chunk, chunk_mode):
    seed = zlib.crc32(f"{fmt}/{variant}/{chunk}".encode()) & 0xFFFF
    size = 300000 + (seed * 41) % 2700000  # 0.3 - 3 MiB
    node = Node(gpu_ctx, oracle_lib, make(fmt, variant, seed, size), fmt, chunk)
    try:
        for stride in STRIDES:
            for front in FRONTS:
                node.walk(stride_views(node.n, stride, front), f"seed={seed} size={node.n} stride={stride} front={front}")
    finally:
        node.free()


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_slab_cuts_from_the_oracle_rows(gpu_ctx, oracle_lib, fmt, chunk_mode):
    chunk = 40000
    seed = zlib.crc32(f"cuts/{fmt}".encode()) & 0xFFFF
    node = Node(gpu_ctx, oracle_lib, make(fmt, "plain", seed, 900000), fmt, chunk)
    try:
        for k in (1, len(node.exp) // 2, len(node.exp) - 2):
            w = window_of_row(node.exp, k, chunk)
            for hi, closes in ((w + WIN, True), (w + WIN - 1, False), (w + 16, False)):
                views = cut_views(node.n, [hi])
                per = node.walk(views, f"seed={seed} k={k} hi={hi}")
                assert per[0] == (k + 1 if closes else k), (per, k, hi)
                if hi == w + WIN - 1:
                    assert views[1][0] == w  # the next slab's window begins exactly at the deferred window
    finally:
        node.free()


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_slab_mid_chunk_carry(gpu_ctx, oracle_lib, fmt, chunk_mode):
    """Windows with no match (FASTQ records of 40-70 KiB, FASTA sequences of 40-90 KiB): cuts after the
    first and after the second unmatched window, and off > curr across two slab ends in a row."""
    chunk = WIN + 1
    seed = zlib.crc32(f"long/{fmt}".encode()) & 0xFFFF
    node = Node(gpu_ctx, oracle_lib, make(fmt, "long", seed, 1200000), fmt, chunk)
    try:
        long_rows = [k for k in range(len(node.exp) - 1) if int(node.exp[k, 1]) >= 2 * WIN + 2]
        assert long_rows, f"seed={seed}: no chunk with two unmatched windows"
        for k in long_rows[:2]:
            curr = int(node.exp[k, 0])
            w0 = curr + chunk - WIN
            for cuts in ([w0 + WIN], [w0 + 2 * WIN], [w0 + WIN, w0 + 2 * WIN]):
                views = cut_views(node.n, cuts)
                got = []
                for i, (lo, hi) in enumerate(views):
                    r = node.slab(lo, hi, first=i == 0)
                    assert r.ok, (seed, k, cuts, r)
                    if r.count:
                        got.append(node.rows.rows(r.count))
                    if i < len(cuts):
                        st = node.carry_state()
                        assert st["curr"] == curr and st["off"] == curr + (cuts[i] - w0), (seed, k, cuts, i, st)
                assert np.array_equal(np.concatenate(got), node.exp), (seed, k, cuts)
                assert node.carry_state()["count"] == len(node.exp)
    finally:
        node.free()


def test_slabs_with_no_window(gpu_ctx, oracle_lib, chunk_mode):
    """The default chunk (1 MiB) over 131072-byte slabs: most calls return OK with 0 rows and leave the
    carry's position where it was."""
    node = Node(gpu_ctx, oracle_lib, make("fastq", "plain", 5, 2500000), "fastq", 0)
    try:
        empty, prev = 0, None
        got = []
        for lo, hi in stride_views(node.n, 131072, 65536):
            r = node.slab(lo, hi)
            assert r.ok
            st = node.carry_state()
            if r.count == 0:
                empty += 1
                if prev is not None:
                    assert (st["curr"], st["off"], st["count"]) == (prev["curr"], prev["off"], prev["count"])
            else:
                got.append(node.rows.rows(r.count))
            prev = st
        assert empty > 10 and np.array_equal(np.concatenate(got), node.exp)
    finally:
        node.free()


def test_slab_ends(gpu_ctx, oracle_lib, chunk_mode):
    base = fastq_records(random.Random(3), 500)
    # a file shorter than chunk: one is_last slab, one row (0, n)
    node = Node(gpu_ctx, oracle_lib, base[:20000], "fastq", WIN)
    per = node.walk([(0, node.n)], "short")
    assert per == [1] and node.exp.tolist() == [[0, node.n]]
    node.free()
    # w + WIN == n exactly and n - 1 (test_exact_eof_boundaries' sizes), the last cut before and after that window
    for size in (WIN - 1, WIN, WIN + 1, 2 * WIN, len(base)):
        node = Node(gpu_ctx, oracle_lib, base[:size], "fastq", WIN)
        for cuts in ([], [size - 1], [max(size - WIN, 16)], [max(size - WIN - 1, 16), size - 1]):
            node.walk(cut_views(node.n, [c for c in cuts if 0 < c < size]), f"size={size} cuts={cuts}")
        node.free()
    # the 32767 clamp (test_match_at_window_end_is_clamped's input), a cut right after the clamped window
    chunk = WIN + 100
    rec, head = b"@a\nAC\n+\n!!\n", b"@h\nA\n+\n!\n"
    pad = chunk - len(head) - len(rec)
    data = head + (b"A" * 60 + b"\n") * (pad // 61) + b"A" * (pad % 61) + rec + b"@z\nA\n+\n!\n" * 4000
    node = Node(gpu_ctx, oracle_lib, data, "fastq", chunk)
    assert int(node.exp[0, 1]) == chunk - 1
    for cuts in ([chunk], [chunk - 1], [chunk + 1]):
        node.walk(cut_views(node.n, cuts), f"clamp cuts={cuts}")
    node.free()


def test_slab_empty_file(gpu_ctx, oracle_lib):
    """n == 0: whatever the whole-node entry returns."""
    buf, rows, carry = gpu_ctx.alloc(64), gpu_ctx.alloc(64), gpu_ctx.chunkrecord_carry()
    for fmt in ("fastq", "fasta", None):
        whole = gpu_ctx.chunkrecord_buffer(buf, 0, rows, fmt=fmt)
        r = gpu_ctx.chunkrecord_slab(buf, 0, 0, 0, 0, carry, rows, fmt=fmt)
        assert (r.status, r.count, r.err) == (whole.status, whole.count, whole.err), (fmt, r, whole)
        if r.ok and r.count:
            assert rows.rows(r.count).tolist() == [[0, 0]]


def test_slab_bad_predictions(gpu_ctx, oracle_lib):
    """A FASTQ record index that fails mid-file, and bytes over the regex alphabet where the record table
    predicts little: the rows are still the oracle's (the speculative mode only)."""
    good = fastq_records(random.Random(77), 9000)
    bad = good[: len(good) // 2] + b"@broken\nACGT\n+\nII\n" + good[len(good) // 2:]
    for chunk in (WIN + 1, 70001):
        node = Node(gpu_ctx, oracle_lib, bad, "fastq", chunk)
        for stride in (262144, 99984):
            node.walk(stride_views(node.n, stride, 65536), f"broken chunk={chunk} stride={stride}")
        node.free()
    rng = random.Random(5)
    alpha = b"@@@++\n\n\r\r ACGTacgt-\t!I>"
    for i in range(10):
        data = bytes(rng.choice(alpha) for _ in range(WIN * 3 + rng.randint(0, 5000)))
        chunk = WIN + 1 + rng.randint(0, 3000)
        for fmt in ("fastq", "fasta"):
            node = Node(gpu_ctx, oracle_lib, data, fmt, chunk)
            node.walk(stride_views(node.n, 49152, 32768), f"fuzz {i} {fmt} chunk={chunk}")
            node.free()


def test_slab_contract(gpu_ctx, oracle_lib, chunk_mode):
    chunk = 40000
    node = Node(gpu_ctx, oracle_lib, make("fastq", "plain", 11, 700000), "fastq", chunk)
    try:
        views = stride_views(node.n, 131072, 65536)
        # a slab whose window starts after the carry's next window: EINVAL, carry unchanged
        r = node.slab(*views[0])
        assert r.ok
        first = node.rows.rows(r.count)
        before = node.carry_state()
        r = node.slab(views[2][0], views[2][1])
        assert r.status == EINVAL and b"before" in r.err and node.carry_state() == before, r
        got = [first]
        for lo, hi in views[1:]:
            r = node.slab(lo, hi)
            assert r.ok
            if r.count:
                got.append(node.rows.rows(r.count))
        assert np.array_equal(np.concatenate(got), node.exp)
        # after the last slab the walk has ended
        assert node.slab(*views[-1]).status == EINVAL
        # row_cap too small: ESPACE with the count the slab needs, carry unchanged; the repeat is right
        r = node.slab(*views[0])
        small = gpu_ctx.alloc(16 * 1)
        before = node.carry_state()
        r = node.slab(*views[1], rows=small)
        need = r.count
        assert r.status == ESPACE and need > 1 and node.carry_state() == before, r
        r = node.slab(*views[1])
        assert r.ok and r.count == need
        n0 = len(first)
        assert np.array_equal(node.rows.rows(need), node.exp[n0:n0 + need])
        small.free()
    finally:
        node.free()
    # SAM through the first slab: EFORMAT with the whole-node text
    sam = b"@HD\tVN:1.0\n" + b"r\t0\t*\n" * 10000
    buf, rows, carry = gpu_ctx.alloc(len(sam) + 64), gpu_ctx.alloc(1024), gpu_ctx.chunkrecord_carry()
    buf.upload(sam)
    whole = gpu_ctx.chunkrecord_buffer(buf, len(sam), rows, fmt="sam")
    r = gpu_ctx.chunkrecord_slab(buf, 0, 0, 40000, len(sam), carry, rows, fmt="sam")
    assert r.status == EFORMAT == whole.status and b"sam.SeekChunk" in r.err and r.err == whole.err, r
    # AUTO with a 16 KiB first window on a larger file: EINVAL
    r = gpu_ctx.chunkrecord_slab(buf, 0, 0, 16384, len(sam), carry, rows, fmt=None)
    assert r.status == EINVAL and b"32 KiB" in r.err, r
    for b in (buf, rows, carry):
        b.free()


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_chunk_fd_walk(gpu_ctx, oracle_lib, tmp_path, fmt, chunk_mode):
    data = make(fmt, "plain", 21, 6 << 20)
    assert len(data) == 6 << 20
    path = tmp_path / "node.data"
    path.write_bytes(data)
    fd = os.open(path, os.O_RDONLY)
    try:
        for chunk in (65536, 0):
            exp, err = oracle_lib.chunkrecord(data, fmt, chunk or oracle_lib.CHUNK_SIZE)
            assert err is None
            for slab_bytes in (1 << 20, 262144):
                r = gpu_ctx.chunkrecord_fd_walk(fd, len(data), fmt=None, chunk=chunk, slab_bytes=slab_bytes)
                assert r.ok and r.path == 6 and r.fmt == fmt and r.count == len(exp), (chunk, slab_bytes, r)
                assert np.array_equal(r.rows, exp), (chunk, slab_bytes)
    finally:
        os.close(fd)
        gpu_ctx.trim(0)


def test_chunk_fd_under_the_cap(oracle_lib, tmp_path, monkeypatch):
    """A 96 MiB FASTQ node under a 32 MiB device cap: Indexers["chunkrecord"] and chunkrecord_fd take
    the walk, the table is the oracle's and the context never holds more than the cap; the same file
    uncapped takes the whole-node path with an equal table."""
    from shock_amd import Context, indexer
    CAP = 32 << 20
    block = fastq_records(random.Random(31), 4200)[: 1 << 20]
    block = block[: block.rfind(b"\n@r") + 1]
    data = block * (96 * 2**20 // len(block))
    exp, err = oracle_lib.chunkrecord(data, "fastq")
    assert err is None and len(exp) > 90
    path = tmp_path / "node.fastq"
    path.write_bytes(data)
    ctx = Context(0)
    fd = os.open(path, os.O_RDONLY)
    try:
        ctx.set_dev_cap(CAP)
        r = ctx.chunkrecord_fd(fd, len(data))
        assert r.ok and r.path == 6 and r.count == len(exp) and np.array_equal(r.rows, exp), r
        assert ctx.workspace_bytes() <= CAP, ctx.workspace_bytes()  # the caches only grow during a walk
        ctx.set_dev_cap(0)
        ctx.trim(0)
        r = ctx.chunkrecord_fd(fd, len(data))
        assert r.ok and r.path != 6 and r.count == len(exp) and np.array_equal(r.rows, exp), r
        assert ctx.workspace_bytes() > len(data)  # the whole node was staged
    finally:
        os.close(fd)
        ctx.close()
    # the registry entry the server calls, through the module's context
    monkeypatch.setattr(indexer, "PATH_DATA", str(tmp_path))
    ictx = indexer.context()
    ictx.trim(0)
    ictx.set_dev_cap(CAP)
    try:
        out = tmp_path / "chunkrecord.idx"
        with open(path, "rb") as f:
            count, ifmt, ierr = indexer.Indexers["chunkrecord"](f).create(str(out))
        assert ierr is None and ifmt == "array" and count == len(exp)
        assert out.read_bytes() == exp.astype("<u8").tobytes()
        assert ictx.workspace_bytes() <= CAP, ictx.workspace_bytes()
    finally:
        ictx.set_dev_cap(0)
        ictx.trim(0)
