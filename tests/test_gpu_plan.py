"""GPU: the download plan (shockidx_download_plan) -- all parts of a ?download&index=X&part=...
request turned into the Streamer's section list on the device -- compared whole (sections, size,
error text, failing part) against tests/planref.py, the transcription of
controller/node/single.go:372-483 over the C restatements of Idx.Part / Idx.Range (parity unpinned
by reference-held vectors, see tests/test_plan_ref.py).  Every case goes through both
Context.download_plan (device pointers) and Context.download_plan_host.
"""
import random

import numpy as np
import pytest

import gen
import planref
import streamref
from planref import CHUNK_RANGE, PART, RANGE, SIZE
from test_oracle_part import ROWS, _random_rows
from test_plan_ref import KATS, case_args, case_expect, table

pytestmark = pytest.mark.gpu
ESPACE = -6
BLOCK = 256    # visits per workgroup of the plan's flag and emit passes (PLAN_THREADS)
SCAN = 2048    # items per workgroup of the flag scan (dscan::BLOCK)
E_NOFILE = b"Index file is missing"


class Dev:
    """index tables uploaded once, plans run over them through both entry points"""

    def __init__(self, ctx, oracle, rows, rec=None):
        self.ctx, self.oracle, self.rows, self.rec = ctx, oracle, rows, rec
        self.bufs = []
        self.d_rows, self.nrows = self._up(rows)
        self.d_rec, self.rec_nrows = self._up(rec)

    def _up(self, t):
        if t is None:
            return None, 0
        t = np.ascontiguousarray(t, dtype=np.uint64).reshape(-1, 2)
        b = self.ctx.alloc(16 * len(t) + 64)
        self.bufs.append(b)
        if len(t):
            b.upload(t.tobytes())
        return b.ptr, len(t)

    def free(self):
        for b in self.bufs:
            b.free()

    def plan(self, mode, parts, il, rl=0, fs=0, cs=0, d_secs=None, cap=0):
        return self.ctx.download_plan(mode, parts, self.d_rows, self.nrows, il, self.d_rec, self.rec_nrows, rl, fs, cs,
                                      d_secs, cap)

    def device(self, mode, parts, il, rl=0, fs=0, cs=0):
        """-> (sections, size, err, err_part) with the sections left on the device, then read back"""
        r = self.plan(mode, parts, il, rl, fs, cs)  # no room: the count comes back with ESPACE
        out = None
        if r.status == ESPACE:
            out = self.ctx.alloc(16 * r.count + 64)
            r = self.plan(mode, parts, il, rl, fs, cs, out.ptr, r.count)
        try:
            if r.status == 1:
                assert (r.count, r.size) == (0, 0)
                return [], 0, r.err, r.err_part
            assert r.status == 0, (r.status, r.err)
            secs = out.rows(r.count).view(np.int64).tolist() if r.count else []
            return secs, planref.i64(r.size), None, r.err_part
        finally:
            if out is not None:
                out.free()

    def check(self, mode, parts, il, rl=0, fs=0, cs=0):
        exp = planref.plan_ref(self.oracle, mode, parts, self.rows, il, self.rec, rl, fs, cs)
        got = self.device(mode, parts, il, rl, fs, cs)
        assert got == exp, (mode, parts[:6], got[1:], exp[1:])
        secs, size, err, ep = self.ctx.download_plan_host(mode, parts, self.rows, il, self.rec, rl, fs, cs)
        assert (secs.tolist(), size, err, ep) == exp, (mode, parts[:6])
        return exp


@pytest.fixture(scope="module")
def rows3000():
    return _random_rows(random.Random(20261020), 3000)


def test_plan_kats_gpu(gpu_ctx, oracle_lib):
    for c in KATS["cases"]:
        mode, parts, rows, il, rec, rl, fs, cs = case_args(c)
        d = Dev(gpu_ctx, oracle_lib, rows, rec)
        try:
            assert d.check(mode, parts, il, rl, fs, cs) == case_expect(c), c["name"]
        finally:
            d.free()


def test_plan_parts_never_merge_gpu(gpu_ctx, oracle_lib):
    d = Dev(gpu_ctx, oracle_lib, ROWS)
    try:
        assert d.check(RANGE, ["1-2", "3-4"], 6)[0] == [[0, 15], [15, 7], [40, 3]]  # rows 2 and 3 touch
        assert d.check(RANGE, ["1-2", "3"], 6)[0] == [[0, 15], [15, 7]]
        for parts in (["1-3", "1-3"], ["1-3", "2-4"], ["2-4", "1-3", "2"], ["6", "5", "4", "3-4", "1-2"],
                      ["4-5", "1-6", "4-5"]):
            d.check(RANGE, parts, 6)
            d.check(PART, parts, 6)
    finally:
        d.free()


def test_plan_range_shapes_in_a_list_gpu(gpu_ctx, oracle_lib):
    """N, N-N, N-(N+1) (the "last record" special case, index.go:161-168) and b < a (empty), each
    between non-empty parts"""
    d = Dev(gpu_ctx, oracle_lib, ROWS)
    try:
        for mid in ("2", "2-2", "2-3", "3-4", "3-2", "6-1", "+2", "2-3-9"):
            exp = d.check(RANGE, ["1-3", mid, "4-6"], 6)
            assert exp[2] is None and exp[0][0] == [0, 22] and exp[0][-2:] == [[40, 5], [100, 1]]
        d.check(RANGE, ["1-3", "3-2", "6-1", "5-4"], 6)
        d.check(RANGE, ["3-2"], 6)
        for bad in ("0", "7", "x", "0-2", "1-7", "-2", "2-", "1 -2", "99999999999999999999-2", ""):
            for k in (0, 1, 2):
                parts = ["1-3", "4", "5-6"]
                parts.insert(k, bad)
                exp = d.check(RANGE, parts, 6)
                assert exp[2] is not None and exp[3] == k
                assert d.check(PART, parts, 6)[3] == k
    finally:
        d.free()


def test_plan_short_file_gpu(gpu_ctx, oracle_lib):
    """A table of 3 rows with idx_length 6: "last row read" holds per part, and a part whose first
    row is past the end reads zeros even right after a part that read rows"""
    d = Dev(gpu_ctx, oracle_lib, ROWS[:3])
    try:
        exp = d.check(RANGE, ["2-6", "5-6", "2-6", "4-6", "1-4"], 6)
        assert exp[0][:5] == [[10, 12], [15, 7], [15, 7], [15, 7], [0, 0]]
        d.check(RANGE, ["5-6", "2-6"], 6)
        d.check(RANGE, ["3-6", "4", "6-6", "3"], 6)
        d.check(PART, ["5", "2-5", "5-2", "4-6", "3"], 6)
        e = Dev(gpu_ctx, oracle_lib, ROWS[:0])  # an empty file
        try:
            e.check(RANGE, ["1-6", "2"], 6)
            e.check(PART, ["1-6", "2"], 6)
        finally:
            e.free()
    finally:
        d.free()


def _seam_parts(rng, n, total=19000):
    """Parts whose ends, laid end to end, fall one before, at and one after every multiple of the
    plan's block and of the scan's block, up to `total` visits"""
    ends = sorted({m + k for step in (BLOCK, SCAN) for m in range(step, total, step) for k in (-1, 0, 1)})
    parts, at = [], 0
    for e in ends:
        ln = e - at
        a = rng.randrange(1, n - ln + 2)
        parts.append(str(a) if ln == 1 and rng.random() < 0.5 else f"{a}-{a + ln - 1}")
        at = e
    return parts


def _small_parts(rng, n, count):
    """count parts of a few rows each (some empty, some in error-free odd spellings)"""
    parts = []
    for _ in range(count):
        a = rng.randrange(1, n - 6)
        c = rng.random()
        parts.append(str(a) if c < 0.2 else f"{a + 2}-{a}" if c < 0.3 else f"+{a}-{a}" if c < 0.35
                     else f"{a}-{a + rng.randrange(0, 7)}")
    return parts


@pytest.mark.parametrize("seed", [1, 2])
def test_plan_seams_gpu(gpu_ctx, oracle_lib, rows3000, seed):
    rng = random.Random(seed)
    d = Dev(gpu_ctx, oracle_lib, rows3000)
    try:
        parts = _seam_parts(rng, 3000)
        assert any("-" not in p for p in parts)
        exp = d.check(RANGE, parts, 3000)
        assert exp[2] is None and len(exp[0]) > len(parts)
        d.check(PART, parts, 3000)
        short = _seam_parts(rng, 3004, 5000)  # the same over a table shorter than its idx_length
        d.check(RANGE, short + ["3001-3004", "2999-3003"], 3004)
    finally:
        d.free()


@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 4096])
def test_plan_part_counts_gpu(gpu_ctx, oracle_lib, rows3000, count):
    rng = random.Random(count)
    d = Dev(gpu_ctx, oracle_lib, rows3000)
    try:
        parts = _small_parts(rng, 3000, count)
        d.check(RANGE, parts, 3000)
        d.check(PART, parts, 3000)
        parts[-1] = "3001"  # the last part fails: nothing is delivered
        assert d.check(RANGE, parts, 3000)[2:] == (b"Index record out of bounds", count - 1)
    finally:
        d.free()


def test_plan_chunk_range_gpu(gpu_ctx, oracle_lib):
    """The constructed matrix index of 5 rows over a record index of 40 (tests/golden/plan): parts
    over 1, 2 and all chunk rows, the errors in Go's order, the missing record index"""
    rec = table("REC")
    d = Dev(gpu_ctx, oracle_lib, table("MAT"), rec)
    try:
        assert d.check(CHUNK_RANGE, ["1", "2"], 5, 40)[0] == [[0, 100], [100, 100]]  # two sections, not one
        for parts in (["1"], ["3"], ["1-2"], ["2-3"], ["4-5"], ["1-5"], ["5", "1-5", "3", "5-1"], ["5"], ["2", "1"],
                      ["1-5", "1-5"], ["4", "5-4", "3-3"]):
            assert d.check(CHUNK_RANGE, parts, 5, 40)[2] is None, parts
        d.check(CHUNK_RANGE, ["1-5"], 5, 39)  # the last record is past rec_length: stop 40 > 39
        d.check(CHUNK_RANGE, ["1", "3-4", "2"], 5, 39)
        d.check(CHUNK_RANGE, ["1-5", "6"], 5, 40)
    finally:
        d.free()
    d = Dev(gpu_ctx, oracle_lib, table("MAT"), rec[:30])  # a record index file shorter than its length
    try:
        d.check(CHUNK_RANGE, ["3-4", "1", "4"], 5, 40)
    finally:
        d.free()
    d = Dev(gpu_ctx, oracle_lib, table("MAT_BAD"), rec)
    try:
        for parts, ep in ((["5", "1"], 1), (["2"], 0), (["5", "5", "3"], 2), (["4"], 0), (["5", "4", "1"], 1),
                          (["1", "9"], 0), (["9", "1"], 0), (["5", "9", "1"], 1), (["5", "1", "9"], 1), (["1-5"], 0),
                          (["5-4", "5", "2-3", "x"], 2)):
            exp = d.check(CHUNK_RANGE, parts, 5, 40)
            assert exp[2] is not None and exp[3] == ep, parts
        assert d.check(CHUNK_RANGE, ["5", "5-4", "5"], 5, 40)[2] is None
    finally:
        d.free()
    d = Dev(gpu_ctx, oracle_lib, table("MAT"), None)  # the record index file is missing
    try:
        assert d.check(CHUNK_RANGE, ["5-4", "3-2"], 5, 40) == ([], 0, None, -1)
        assert d.check(CHUNK_RANGE, ["5-4", "5"], 5, 40) == ([], 0, E_NOFILE, 1)
        assert d.check(CHUNK_RANGE, ["5-4", "3-2", "9"], 5, 40)[3] == 2
        assert d.check(CHUNK_RANGE, ["1", "9"], 5, 40) == ([], 0, E_NOFILE, 0)
    finally:
        d.free()


def test_plan_chunk_range_seams_gpu(gpu_ctx, oracle_lib, rows3000):
    """Level-2 segments that cross the block seams: matrix rows over a record index of 3000 rows"""
    mat = np.array([[16 * a, 16 * n] for a, n in ((0, 255), (255, 2), (300, 1793), (2093, 1), (2500, 500), (10, 0),
                                                  (1000, 2000), (2999, 1))], dtype=np.uint64)
    d = Dev(gpu_ctx, oracle_lib, mat, rows3000)
    try:
        exp = d.check(CHUNK_RANGE, ["1", "2", "3", "4", "5", "6", "7", "8"], 8, 3000)
        assert exp[2] is None and len(exp[0]) > 100
        d.check(CHUNK_RANGE, ["1-8"], 8, 3000)
        d.check(CHUNK_RANGE, ["7", "3-4", "8", "1-2", "7"], 8, 3000)
        d.check(CHUNK_RANGE, ["7", "3", "5"], 8, 2999)  # part 0 and 2 end past rec_length
    finally:
        d.free()
    d = Dev(gpu_ctx, oracle_lib, mat, rows3000[:2000])  # "last row read" per level-2 segment
    try:
        d.check(CHUNK_RANGE, ["7", "5", "3", "8"], 8, 3000)
    finally:
        d.free()


def test_plan_size_gpu(gpu_ctx, oracle_lib):
    MiB = 1 << 20
    d = Dev(gpu_ctx, oracle_lib, None)
    try:
        size = 5 * MiB + 12345
        for cs in (MiB, 1, 0, -1):
            for parts in (["1", "6", "5", "2-3"], ["6-6", "5-6", "1-6"], ["7"], ["1", "1-7"], ["5-9"], ["3-1"],
                          [str(size), str(size + 1), f"{size}-{size + 1}"], [str(size + 2)], ["0"], ["x", "1"]):
                d.check(SIZE, parts, 0, 0, size, cs)
        d.check(SIZE, ["5", "3", "3-5", "2"], 0, 0, 10, 1 << 62)  # products that wrap int64
        d.check(SIZE, ["9223372036854775807", "2"], 0, 0, 9, 2)
        d.check(SIZE, ["2", "3"], 0, 0, 9, -(1 << 63))
        d.check(SIZE, ["1"], 0, 0, 0, MiB)
    finally:
        d.free()


def test_plan_capacity_gpu(gpu_ctx, oracle_lib):
    """secs_cap one short: ESPACE with the count needed and d_secs untouched; no parts; missing files"""
    rec = table("REC")
    d = Dev(gpu_ctx, oracle_lib, table("MAT"), rec)
    guard = gpu_ctx.alloc(16 * 64)
    try:
        for mode, parts, il, rl, fs, cs in ((PART, ["1", "2-3", "5"], 5, 0, 0, 0), (RANGE, ["1-5", "2"], 5, 0, 0, 0),
                                            (CHUNK_RANGE, ["1-5", "3"], 5, 40, 0, 0), (SIZE, ["1", "2"], 0, 0, 99, 10)):
            exp = planref.plan_ref(oracle_lib, mode, parts, d.rows, il, rec, rl, fs, cs)
            need = len(exp[0])
            assert need >= 2
            guard.fill(0xAB)
            r = d.plan(mode, parts, il, rl, fs, cs, guard.ptr, need - 1)
            assert (r.status, r.count, r.err_part) == (ESPACE, need, -1), mode
            assert bytes(guard.download()) == b"\xab" * (16 * 64), mode
            r = d.plan(mode, parts, il, rl, fs, cs, guard.ptr, need)  # exactly enough
            assert (r.status, r.count, planref.i64(r.size)) == (0, need, exp[1])
            assert guard.rows(need).view(np.int64).tolist() == exp[0]
            assert bytes(guard.download(16 * 64 - 16 * need, 16 * need)) == b"\xab" * (16 * 64 - 16 * need)
            assert d.check(mode, [], il, rl, fs, cs) == ([], 0, None, -1)  # nparts == 0
    finally:
        guard.free()
        d.free()
    d = Dev(gpu_ctx, oracle_lib, None, rec)  # the index named in the request is missing
    try:
        for mode in (PART, RANGE, CHUNK_RANGE):
            assert d.check(mode, ["x", "1"], 5, 40) == ([], 0, E_NOFILE, 0)
            assert d.check(mode, [], 5, 40) == ([], 0, None, -1)
        assert d.check(SIZE, ["1"], 0, 0, 99, 10) == ([[0, 10]], 10, None, -1)  # the size index has no file
    finally:
        d.free()


def test_plan_to_stream_on_device_gpu(gpu_ctx, oracle_lib):
    """A 4 MiB FASTQ node: its record index, a subset node, the subset's chunkrecord matrix index, the
    plan of parts ["1", "2-3"] and the sectioned stream over its sections -- the sections never visit
    the host between the plan and the stream"""
    ctx = gpu_ctx
    data = gen.fq_uniform(250, 4 << 20, extra=3)
    r = ctx.build_host(data, "record", "fastq")
    assert r.ok
    parent, R = r.rows, r.count
    ids = "".join(f"{i}\n" for i in range(1, R + 1) if i % 37).encode()  # a gap after every 36 records
    d_ids, d_par, d_data = ctx.alloc(len(ids) + 64), ctx.alloc(16 * R + 64), ctx.alloc(len(data) + 64)
    d_ids.upload(ids)
    d_par.upload(parent.tobytes())
    d_data.upload(data)
    d_sub, d_runs, d_mat = ctx.alloc(16 * R + 64), ctx.alloc(16 * R + 64), ctx.alloc(16 * 64)
    d_secs, d_out = ctx.alloc(16 * R + 64), ctx.alloc(2 * len(data) + 64)
    try:
        sn = ctx.subset_index(d_ids.ptr, len(ids), d_par.ptr, R, R, d_sub.ptr, R, d_runs.ptr, R)
        assert sn.ok and sn.count == R - R // 37
        K = sn.count
        m = ctx.chunkrecord_subset_device(d_sub.ptr, K, d_mat.ptr, 64)
        assert m.ok and m.count >= 3
        M = m.count
        parts = ["1", "2-3"]
        p = ctx.download_plan(CHUNK_RANGE, parts, d_mat.ptr, M, M, d_sub.ptr, K, K, 0, 0, d_secs.ptr, R)
        assert p.ok and p.err_part == -1
        sub, mat = d_sub.rows(K), d_mat.rows(M)
        exp = planref.plan_ref(oracle_lib, CHUNK_RANGE, parts, mat, M, sub, K)
        assert exp[2] is None and (p.count, planref.i64(p.size)) == (len(exp[0]), exp[1]) and p.count > BLOCK
        assert d_secs.rows(p.count).view(np.int64).tolist() == exp[0]
        raw = ctx.stream_filter_device(None, d_data.ptr, len(data), d_secs.ptr, p.count, d_out.ptr, 2 * len(data))
        assert raw.ok and raw.size == p.size
        assert d_out.download(raw.size).tobytes() == b"".join(data[a:a + n] for a, n in exp[0])
        out, count, err, _ = streamref.stream_ref(oracle_lib, "fq2fa", data, exp[0])
        assert err is None
        f = ctx.stream_filter_device("fq2fa", d_data.ptr, len(data), d_secs.ptr, p.count, d_out.ptr, 2 * len(data))
        assert (f.status, f.count, f.size, f.err_section) == (0, count, len(out), -1)
        assert d_out.download(f.size).tobytes() == out
    finally:
        for b in (d_ids, d_par, d_data, d_sub, d_runs, d_mat, d_secs, d_out):
            b.free()


def test_download_module_gpu(gpu_ctx, oracle_lib, tmp_path):
    """shock_amd.download over .idx files: the four modes, the full-file forms and the controller's
    own errors (single.go:343-484)"""
    from shock_amd.core import write_idx
    from shock_amd.download import Download
    from shock_amd.stream import DeviceSections
    rec, mat = table("REC"), table("MAT")
    p_rows, p_rec, p_mat = (str(tmp_path / n) for n in ("rows.idx", "record.idx", "chunkrecord.idx"))
    write_idx(ROWS, str(tmp_path), p_rows)
    write_idx(rec, str(tmp_path), p_rec)
    write_idx(mat, str(tmp_path), p_mat)
    missing = str(tmp_path / "missing.idx")

    def same(got, exp):
        s, err = got
        if exp[2] is not None:
            assert s is None and err.msg == exp[2] and err.part == exp[3]
        else:
            assert err is None and isinstance(s.R, DeviceSections)
            assert ([list(x) for x in s.R.tolist()], s.Size) == exp[:2]

    ref = planref.plan_ref
    for parts in (["2-3", "6-1", "1"], ["1", "9"]):  # PART: a non-subset index of a file
        same(Download("basic", "record", "record", 6, p_rows, parts, file_size=101), ref(oracle_lib, PART, parts, ROWS, 6))
    same(Download("basic", "record", "record", 6, missing, ["1"], file_size=101), ([], 0, E_NOFILE, 0))
    s, err = Download("basic", "record", "record", 6, p_rows, ["1"], file_size=0)  # :463-466 an empty node
    assert s is None and err.msg == b"Index record out of bounds"
    s, err = Download("basic", "record", "record", 6, p_rows)  # :477-482
    assert s is None and err.msg == b"Index parameter requires part parameter"
    for parts in (["1-2", "3-4"], ["4-5", "7"]):  # RANGE: a subset index
        same(Download("basic", "sub", "subset", 6, p_rows, parts, file_size=101), ref(oracle_lib, RANGE, parts, ROWS, 6))
    same(Download("basic", "sub", "subset", 6, p_rows), ref(oracle_lib, RANGE, ["1-6"], ROWS, 6))  # :433-445
    for parts in (["1", "2"], ["1-5"], ["6"]):  # CHUNK_RANGE: a subset node's chunkrecord index
        same(Download("subset", "chunkrecord", "chunkrecord", 5, p_mat, parts, record_total_units=40,
                      record_idx_path=p_rec), ref(oracle_lib, CHUNK_RANGE, parts, mat, 5, rec, 40))
    same(Download("subset", "chunkrecord", "chunkrecord", 5, p_mat, ["5-4", "1"], record_total_units=40,
                  record_idx_path=missing), ([], 0, E_NOFILE, 1))
    same(Download("subset", "chunkrecord", "chunkrecord", 5, p_mat, record_total_units=40, record_idx_path=p_rec),
         ref(oracle_lib, RANGE, ["1-40"], rec, 40))  # :388-400 the full subset file
    s, err = Download("subset", "chunkrecord", "chunkrecord", 5, p_mat, ["1"])  # :375-380
    assert s is None and err.msg == (b"Invalid request, record index must exist to retrieve chunkrecord index "
                                     b"on a subset node.")
    for cs, parts in ((None, ["1", "3", "2-3"]), (1000, ["1", "2622"]), (0, ["4"]), (1000, ["2623"])):  # SIZE
        exp = ref(oracle_lib, SIZE, parts, None, 0, None, 0, 2621440, 1048576 if cs is None else cs)
        same(Download("basic", "size", "virtual", 0, "", parts, file_size=2621440, chunk_size=cs), exp)
    s, err = Download("subset", "size", "virtual", 0, "", ["1"], file_size=10)  # :351-355
    assert s is None and err.msg == b"subset nodes do not currently support virtual indices"
    # the Streamer over device-resident sections: the bytes the client receives
    node = b"@a\nAC\n+\nII\n@b\nG\n+\nJ\n@c\nGG\n+\nJ\n"
    p_node = str(tmp_path / "node.idx")
    write_idx(np.array([[0, 11], [11, 9], [20, 10]], dtype=np.uint64), str(tmp_path), p_node)
    s, err = Download("basic", "record", "record", 3, p_node, ["2", "1"], file_size=len(node), Filter="anonymize")
    assert err is None and s.Size == 20 and s.Stream(node).read() == b"@1\nG\n+\nJ\n@1\nAC\n+\nII\n" and s.E is None
    s, err = Download("basic", "record", "record", 3, p_node, ["1-2", "2"], file_size=len(node))
    assert err is None and s.R.tolist() == [(0, 20), (11, 9)] and s.Stream(node).read() == node[:20] + node[11:20]
    s, err = Download("basic", "sub", "subset", 3, p_node, ["3-2"], file_size=len(node))
    assert err is None and len(s.R) == 0 and s.Size == 0 and s.Stream(node).read() == b""
