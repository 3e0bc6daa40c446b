"""The subset indexes from files: shockidx_subset_fd_walk (always slab by slab) and
shockidx_subset_create (the whole build within the device budget, else the walk; temp files and
renames as index/subset.go:136-158,274-297) against the oracle on the whole input."""
import os

import numpy as np
import pytest

from test_gpu_subset_slabs import P4096, SPARSE, DENSE, parent_table, text

pytestmark = pytest.mark.gpu

EFORMAT = 1


def _files(tmp_path, ids: bytes, parent, tail: bytes = b""):
    """the id list and the parent index as files (tail: bytes of a last, partial parent row)"""
    pi, pp = tmp_path / "ids.txt", tmp_path / "parent.idx"
    pi.write_bytes(ids)
    pp.write_bytes(np.ascontiguousarray(parent, dtype="<u8").tobytes() + tail)
    return str(pi), str(pp)


def _walk(ctx, ids_path, par_path, ilength, **kw):
    fi, fp = os.open(ids_path, os.O_RDONLY), os.open(par_path, os.O_RDONLY)
    try:
        return ctx.subset_fd_walk(fi, os.fstat(fi).st_size, fp, os.fstat(fp).st_size, ilength, **kw)
    finally:
        os.close(fi)
        os.close(fp)


def _create(ctx, ids_path, par_path, ilength, tmpdir, cofile, ofile):
    fi, fp = os.open(ids_path, os.O_RDONLY), os.open(par_path, os.O_RDONLY)
    try:
        return ctx.subset_create(fi, os.fstat(fi).st_size, fp, os.fstat(fp).st_size, ilength, tmpdir, cofile, ofile)
    finally:
        os.close(fi)
        os.close(fp)


def _idx_bytes(rows):
    return np.ascontiguousarray(rows, dtype="<u8").tobytes()


BIG = sorted(set(np.random.default_rng(23).integers(1, 4097, 3000).tolist()))  # ~11 KB of text


def test_fd_walk_explicit_sizes(gpu_ctx, oracle_lib, tmp_path):
    ids = text(list(range(1, 20000, 3)), blank_every=11) + text(list(range(20000, 40000, 2)))  # ~100 KB: two 64 KiB slabs
    par = parent_table(40000, seed=29)
    pi, pp = _files(tmp_path, ids, par, tail=b"\x01\x02\x03")  # a partial last row is no row
    rows, runs, size, err = oracle_lib.subset(ids, par)
    assert err is None and len(ids) > 65536
    r = _walk(gpu_ctx, pi, pp, len(par), ids_slab_bytes=65536, parent_slab_rows=4096)
    assert r.ok and (r.count, r.runs, r.size) == (len(rows), len(runs), size)
    assert np.array_equal(r.rows, rows) and np.array_equal(r.run_rows, runs)
    st = gpu_ctx.subset_stats()
    assert st["walked"] == 1 and st["slabs"] == -(-len(ids) // 65536) and st["windows"] >= 40000 // 4096
    assert st["calls"] >= st["slabs"] + st["windows"] - 1 and st["slab_bytes"] == 65536 and st["window_rows"] == 4096
    # without runs: CreateSubsetIndex's table
    rows2, count2, size2, err2 = oracle_lib.create_subset_index(ids, par)
    r = _walk(gpu_ctx, pi, pp, len(par), want_runs=False, ids_slab_bytes=65536, parent_slab_rows=4096)
    assert r.ok and (r.count, r.runs, r.size) == (count2, 0, size2) and np.array_equal(r.rows, rows2)
    # an error in the second slab: Go's text, the totals and the tables at that point
    cut = ids.rfind(b"\n", 0, 80000) + 1
    bad = ids[:cut] + b"17\n" + ids[cut:]
    pi, pp = _files(tmp_path, bad, par)
    rows, runs, size, err = oracle_lib.subset(bad, par)
    assert err is not None and err.startswith(b"Subset indices must be")
    r = _walk(gpu_ctx, pi, pp, len(par), ids_slab_bytes=65536, parent_slab_rows=4096)
    assert r.status == EFORMAT and r.err == err and (r.count, r.runs, r.size) == (len(rows), len(runs), size)
    assert np.array_equal(r.rows, rows) and np.array_equal(r.run_rows, runs)


def test_create_files(gpu_ctx, oracle_lib, tmp_path):
    tmpdir = tmp_path / "temp"
    tmpdir.mkdir()
    ids = text(BIG, blank_every=13)
    pi, pp = _files(tmp_path, ids, P4096)
    rows, runs, size, err = oracle_lib.subset(ids, P4096)
    co, o = str(tmp_path / "n.subset.idx"), str(tmp_path / "record.idx")
    r = _create(gpu_ctx, pi, pp, 4096, str(tmpdir), co, o)
    assert r.ok and (r.count, r.runs, r.size) == (len(rows), len(runs), size)
    assert open(o, "rb").read() == _idx_bytes(rows) and open(co, "rb").read() == _idx_bytes(runs)
    assert os.listdir(tmpdir) == [] and gpu_ctx.subset_stats()["walked"] == 0
    # cofile None: CreateSubsetIndex
    o2 = str(tmp_path / "only.idx")
    r = _create(gpu_ctx, pi, pp, 4096, str(tmpdir), None, o2)
    assert r.ok and (r.count, r.runs, r.size) == (len(rows), 0, size)
    assert open(o2, "rb").read() == _idx_bytes(rows) and os.listdir(tmpdir) == []
    # an empty id file: two empty tables
    pe = str(tmp_path / "empty.txt")
    open(pe, "wb").close()
    co3, o3 = str(tmp_path / "e.subset.idx"), str(tmp_path / "e.idx")
    r = _create(gpu_ctx, pe, pp, 4096, str(tmpdir), co3, o3)
    assert r.ok and (r.count, r.runs, r.size) == (0, 0, 0)
    assert os.path.getsize(co3) == 0 and os.path.getsize(o3) == 0 and os.listdir(tmpdir) == []


@pytest.mark.parametrize("bad", [b"12x\n", b"99999999999999999999\n", b"2\n", b"4090\n", b"4097\n"])
def test_create_errors_leave_nothing(gpu_ctx, oracle_lib, tmp_path, bad):
    """each error kind (Atoi's two, the order, an id above ilength, an id above the parent's rows), met after
    rows were written: both paths absent, tmpdir empty"""
    tmpdir = tmp_path / "temp"
    tmpdir.mkdir()
    ids = text(BIG[:2000]) + bad + text(BIG[2000:])
    il = 4080 if bad == b"4090\n" else 5000
    pi, pp = _files(tmp_path, ids, P4096)
    rows, runs, size, err = oracle_lib.subset(ids, P4096, il)
    assert err is not None
    co, o = str(tmp_path / "n.subset.idx"), str(tmp_path / "record.idx")
    r = _create(gpu_ctx, pi, pp, il, str(tmpdir), co, o)
    assert r.status == EFORMAT and r.err == err and (r.count, r.runs, r.size) == (len(rows), len(runs), size)
    assert not os.path.exists(co) and not os.path.exists(o) and os.listdir(tmpdir) == []
    r = _create(gpu_ctx, pi, pp, il, str(tmpdir), None, o)  # (-1, -1, err)
    assert r.status == EFORMAT and r.err == err and r.count == r.size == 2**64 - 1 and r.runs == 0
    assert not os.path.exists(o) and os.listdir(tmpdir) == []


def test_capped_context_takes_the_walk(shockidx_so, oracle_lib, tmp_path):
    """a 3 MiB id list (about 400 k ids) over a 500 k-row parent under a 32 MiB cap: the whole build
    would hold over 50 MB, so the walk runs, within the cap; uncapped, the whole build gives the same bytes"""
    from shock_amd.core import Context
    tmpdir = tmp_path / "temp"
    tmpdir.mkdir()
    rng = np.random.default_rng(31)
    picks = np.flatnonzero(rng.random(500000) < 0.9) + 1
    ids = b"".join(b"%d\n" % i for i in picks.tolist())
    assert 3_000_000 < len(ids) < 3_300_000 and len(picks) > 400_000
    lens = rng.integers(0, 400, 500000).astype(np.uint64)
    gaps = (rng.random(500000) < 0.1).astype(np.uint64) * 7
    offs = np.cumsum(lens + gaps) - lens
    par = np.stack([offs, lens], axis=1)
    pi, pp = _files(tmp_path, ids, par)
    rows, runs, size, err = oracle_lib.subset(ids, par)
    assert err is None
    cap = 32 << 20
    out = {}
    for name, c in (("capped", cap), ("free", 0)):
        ctx = Context(0)
        try:
            if c:
                ctx.set_dev_cap(c)
            co, o = str(tmp_path / (name + ".subset.idx")), str(tmp_path / (name + ".idx"))
            r = _create(ctx, pi, pp, len(par), str(tmpdir), co, o)
            st = ctx.subset_stats()
            assert r.ok and (r.count, r.runs, r.size) == (len(rows), len(runs), size)
            assert st["walked"] == (1 if c else 0), st
            if c:
                assert st["slabs"] > 1 and st["held_bytes"] <= cap and ctx.workspace_bytes() <= cap, st
            out[name] = (open(o, "rb").read(), open(co, "rb").read())
        finally:
            ctx.close()
    assert out["capped"] == out["free"] == (_idx_bytes(rows), _idx_bytes(runs))
    assert os.listdir(tmpdir) == []


def test_python_mirror_takes_the_file_entry(gpu_ctx, oracle_lib, tmp_path, monkeypatch):
    """shock_amd.subset over paths goes through shockidx_subset_create (the context's subset stats move, the
    temp files live under PATH_DATA/temp); a file object goes the old way (they do not move)"""
    from shock_amd import indexer, subset
    monkeypatch.setattr(subset, "PATH_DATA", str(tmp_path / "data"))
    ctx = indexer.context()
    ids = text(SPARSE, blank_every=3)
    pi, pp = _files(tmp_path, ids, P4096)
    rows, runs, size, err = oracle_lib.subset(ids, P4096)
    other = tmp_path / "other.txt"
    other.write_bytes(b"7\n")

    def mark():  # a create over another id file: the stats then say 2 bytes of ids
        assert subset.CreateSubsetIndex(str(other), str(tmp_path / "mark.idx"), pp, "array", 4096)[2] is None
        assert ctx.subset_stats()["ids_bytes"] == 2

    for k, by_path in enumerate((True, False)):
        co, o = str(tmp_path / f"m{k}.subset.idx"), str(tmp_path / f"m{k}.idx")
        mark()
        src = pi if by_path else open(pi, "rb")
        assert subset.CreateSubsetNodeIndexes(src, co, o, pp, "array", 4096) == (len(runs), len(rows), size, None)
        assert open(o, "rb").read() == _idx_bytes(rows) and open(co, "rb").read() == _idx_bytes(runs)
        st = ctx.subset_stats()
        assert (st["ids_bytes"], st["parent_bytes"]) == ((len(ids), 65536) if by_path else (2, 65536))
        mark()
        src = pi if by_path else open(pi, "rb")
        assert subset.CreateSubsetIndex(src, o + "x", pp, "array", 4096) == (len(rows), size, None)
        assert open(o + "x", "rb").read() == _idx_bytes(rows)
        assert ctx.subset_stats()["ids_bytes"] == (len(ids) if by_path else 2)
    assert os.listdir(tmp_path / "data" / "temp") == []
    # the error conventions: a missing parent index is (-1, -1, err) for CreateSubsetIndex, a missing id file raises
    c, s_, err = subset.CreateSubsetIndex(pi, str(tmp_path / "no.idx"), str(tmp_path / "missing.idx"), "array", 4096)
    assert (c, s_) == (-1, -1) and err is not None
    with pytest.raises(OSError):
        subset.CreateSubsetIndex(str(tmp_path / "missing.txt"), str(tmp_path / "no.idx"), pp, "array", 4096)
    assert DENSE  # (shared with the slab tests)
