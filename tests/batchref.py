"""Helpers of tests/test_gpu_batch.py: the expected result of every node of a batch from the oracle
(oracle.record_index / oracle.line_index over the node's bytes alone), arenas packed the way
shockidx_build_batch_device wants them (16-byte aligned nodes, any bytes in between), and the full
comparison of a batch against its expectation -- every node, no filter."""
from __future__ import annotations

import numpy as np

import gen

S = 1024          # the batched walk's step: 64 lanes x 16 bytes (BATCH_STEP, shock_amd/csrc/sidx_batch.hpp)
MARGIN = 64       # arena bytes before the first and after the last node
NO_FORMAT = b"Invalid file type for filter"
OK, EFORMAT, EINVAL, ESPACE = 0, 1, -1, -6


def expect(oracle, body: bytes, kind: str, fmt):
    """(count, format name, status, err, rows) of one node indexed alone."""
    if kind == "line":
        rows, _ = oracle.line_index(body)
        return len(rows), "line", OK, None, rows
    name = fmt if fmt is not None else oracle.detect(body)[0]
    if name is None:
        return 0, None, EFORMAT, NO_FORMAT, np.zeros((0, 2), np.uint64)
    rows, err = oracle.record_index(body, name)
    return len(rows), name, (OK if err is None else EFORMAT), err, rows


def pack(bodies, fill: bytes = b"\0", order=None):
    """-> (arena, nodes [(pos, len)] in list order).  Nodes are placed in `order` (a permutation of the
    list, default list order) at 16-byte aligned positions, MARGIN bytes before the first and after the
    last; every byte that belongs to no node is taken from `fill` repeated."""
    order = list(range(len(bodies))) if order is None else list(order)
    pos = [0] * len(bodies)
    off = MARGIN
    for i in order:
        pos[i] = off
        off = (off + len(bodies[i]) + 15) & ~15
    total = off + MARGIN
    arena = bytearray((fill * (total // len(fill) + 1))[:total])
    for i, b in enumerate(bodies):
        arena[pos[i]:pos[i] + len(b)] = b
    return bytes(arena), [(pos[i], len(b)) for i, b in enumerate(bodies)]


def row_bound(nodes) -> int:
    """More rows than any index of these nodes has (a line index has a row per byte and one more)."""
    return sum(n + 1 for _, n in nodes) + 16


class Batch:
    """One device call over an arena: the BatchResult and the table downloaded from the device."""

    def __init__(self, ctx, arena: bytes, nodes, kind="record", fmt=None, row_cap=None, pattern=None):
        self.d_data = ctx.alloc(len(arena) + 64)
        self.d_data.upload(arena)
        nd = np.array(nodes, dtype=np.int64).reshape(-1, 2)
        self.d_nodes = ctx.alloc(nd.nbytes + 64)
        if nd.size:
            self.d_nodes.upload(nd)
        cap = row_bound(nodes) if row_cap is None else row_cap
        self.d_rows = ctx.alloc(16 * cap + 64)
        if pattern is not None:
            self.d_rows.fill(pattern)
        self.cap = cap
        self.res = ctx.build_batch_device(self.d_data.ptr, len(arena), self.d_nodes.ptr, len(nodes), self.d_rows.ptr,
                                          cap, kind, fmt)
        self.stats = ctx.batch_stats()

    def table(self) -> np.ndarray:
        return self.d_rows.download(16 * self.cap).view("<u8").reshape(-1, 2)

    def free(self):
        for b in (self.d_data, self.d_nodes, self.d_rows):
            b.free()


def compare(res, table, exps, tag):
    """Every node of the batch against its expectation, in full: count, format, status, error bytes
    and all rows; the regions' order and the table's extent."""
    assert res.status == OK, (tag, res.status, res.err)
    assert len(res.items) == len(exps), (tag, len(res.items), len(exps))
    end = 0
    for i, (it, (count, name, status, err, rows)) in enumerate(zip(res.items, exps)):
        where = (tag, "node", i)
        assert (it.count, it.fmt, it.status, it.err) == (count, name, status, err), where
        assert it.row_off >= end, where
        got = table[it.row_off:it.row_off + it.count]
        assert np.array_equal(got, rows), (where, got[:4], rows[:4])
        end = it.row_off + it.count
    assert res.rows_total >= end, tag
    assert res.count == sum(1 for e in exps if e[2] == OK), tag


def run_and_compare(ctx, oracle, bodies, kind, fmt, tag, fill=b"\0", order=None, exps=None):
    """One device call over the packed bodies, compared in full; -> (its items, its stats)."""
    arena, nodes = pack(bodies, fill, order)
    if exps is None:
        exps = [expect(oracle, b, kind, fmt) for b in bodies]
    b = Batch(ctx, arena, nodes, kind, fmt)
    try:
        compare(b.res, b.table(), exps, tag)
        return b.res.items, b.stats
    finally:
        b.free()


# ---- bodies ---------------------------------------------------------------------------------------
def whole_fastq(rng, nbytes: int) -> bytes:
    """Valid random records up to about nbytes."""
    out = b""
    while len(out) < nbytes:
        out += gen.fastq(rng, 1, crlf=0.1, plus_id=0.3)
    return out


def text_of(rng, name: str, nbytes: int) -> bytes:
    """At least nbytes of valid text of a format."""
    if name == "fastq":
        return whole_fastq(rng, nbytes)
    if name == "fasta":
        out = b""
        while len(out) < nbytes:
            out += gen.fasta(rng, 2)
        return out
    if name == "sam":
        return gen.sam(rng, nbytes // 60 + 2, headers=2)
    out = b""
    while len(out) < nbytes:
        out += gen.lines(rng, 8)
    return out


def sized(rng, name: str, n: int, final_nl: bool) -> bytes:
    """A node of exactly n bytes of a format's text whose last byte is / is not a '\\n'."""
    if name == "fastq" and final_nl and (n == 0 or n >= 9):
        return gen.fq_fill(n)
    if name == "fastq" and not final_nl and n >= 8:
        return gen.fq_fill(n + 1)[:-1]
    body = bytearray(text_of(rng, name, n + 1)[:n])
    if n:
        body[-1] = 0x0A if final_nl else 0x41
    return bytes(body)
