"""The subset indexes' slab pass (shockidx_subset_slab_device) through the driver of subslab.py
against the oracle on the whole input (index/subset.go:133-303 and :36-128): the calls' rows and
runs concatenated, the running totals and Go's error text, whatever the id slab size, the cut,
the parent window and the tables' capacities."""
import numpy as np
import pytest

import subslab

pytestmark = pytest.mark.gpu

EINVAL, ESPACE, EFORMAT = -1, -6, 1


def parent_table(n, seed=1, zero=False):
    """n rows: contiguous stretches of random length, broken by gaps; some rows of length 0."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 2), np.uint64)
    off = 0
    for i in range(n):
        if rng.random() < 0.15:
            off += int(rng.integers(1, 50))  # a broken stretch
        ln = 0 if (zero or rng.random() < 0.05) else int(rng.integers(1, 300))
        rows[i] = (off, ln)
        off += ln
    return rows


def text(ids, width=0, blank_every=0, final_newline=True):
    out = []
    for k, i in enumerate(ids):
        if blank_every and k % blank_every == 0:
            out.append(b"\n")
        out.append((b"%0*d\n" % (width, i)) if width else (b"%d\n" % i))
    t = b"".join(out)
    return t if final_newline else t[:-1]


def check(ctx, oracle_lib, ids, parent, ilength=None, **kw):
    rows, runs, size, err = oracle_lib.subset(ids, parent, ilength)
    w = subslab.walk(ctx, ids, parent, ilength, **kw)
    assert w.err == err, (w.err, err, w.log[-3:])
    assert w.outcome == ("ok" if err is None else "err")
    assert np.array_equal(w.rows, rows), (len(w.rows), len(rows))
    assert np.array_equal(w.runs, runs), (w.runs[:8], runs[:8], len(w.runs), len(runs))
    assert (w.count, w.nruns, w.size) == (len(rows), len(runs), size)
    # the protocol: a window never starts before the id that asked for it
    for a, b in zip(w.log, w.log[1:]):
        if a["status"] == 0 and a["stop"] == 2:
            assert b["prow0"] == a["next_id"] - 1 and b["lo"] == a["lo"]
    # ... and every call consumes at least one line: it delivers a row or moves next_off on.  The one
    # call that cannot is the first on a new slab whose first id lies outside the window that the
    # slab before it left behind (nobody has read that id yet): it stops at once, names the id, and
    # the call after it, against the window it asked for, consumes it.
    at, idle, lo = 0, False, None
    for e in w.log:
        if e["status"] != 0 or e["n"] == 0:  # (an empty id text has no line)
            continue
        moved = e["rows"] > 0 or e["next_off"] > at
        if not moved:
            assert e["stop"] == 2 and not idle and lo != e["lo"], e
        idle, at, lo = not moved, e["next_off"], e["lo"]
    return w


SPARSE = sorted(set(np.random.default_rng(7).integers(1, 4097, 900).tolist()))
DENSE = list(range(5, 1500))
P4096 = parent_table(4096)


@pytest.mark.parametrize("slab", [64, 1000, 1024, 4097, 1 << 20])
@pytest.mark.parametrize("window", [3, 64, 65, 0])
def test_slab_sizes_and_windows(gpu_ctx, oracle_lib, slab, window):
    for ids in (text(SPARSE, blank_every=7), text(DENSE, final_newline=False)):
        w = check(gpu_ctx, oracle_lib, ids, P4096, slab_bytes=slab, window_rows=window)
        if window == 3 and ids.startswith(b"\n"):  # the sparse list skips rows of the parent index
            seen = {(e["prow0"], e["prows"]) for e in w.log}
            assert sum(k for _, k in seen) < 4096 // 2


def test_window_of_one_row(gpu_ctx, oracle_lib):
    """every id stops the call once: one id consumed per call"""
    ids = text(SPARSE[:200], blank_every=5)
    w = check(gpu_ctx, oracle_lib, ids, P4096, slab_bytes=257, window_rows=1)
    assert sum(e["rows"] for e in w.log) == 200 and max(e["rows"] for e in w.log) == 1
    par8 = parent_table(8, seed=3)
    check(gpu_ctx, oracle_lib, b"1\n2\n3\n5\n8\n", par8, slab_bytes=4, window_rows=1)


@pytest.mark.parametrize("halo", [0, 3, 65536])
def test_every_cut(gpu_ctx, oracle_lib, halo):
    """a cut just after a '\\n', just before one, inside a number, blank lines at both sides of it,
    and inside the final line without '\\n' -- every slab size from 1 byte to the whole text"""
    par = parent_table(4096, seed=5)
    for ids in (b"10\n20\n\n\n300\n\n4000\n4001\n\n", b"\n\n7\n\n\n123\n2000\n\n3999", b"12\n13\n14\n15"):
        for slab in range(1 if halo >= 5 else 5, len(ids) + 1):  # (a slot holds the longest line, 5 bytes)
            check(gpu_ctx, oracle_lib, ids, par, slab_bytes=slab, halo=halo, window_rows=64)


@pytest.mark.parametrize("k", [63, 64, 65, 256, 257])
def test_wave_and_workgroup_edges(gpu_ctx, oracle_lib, k):
    """slabs holding exactly k non-blank ids (6-byte lines): the check pass's wave and block edges"""
    ids = text(list(range(2, 4000, 3)), width=5)
    w = check(gpu_ctx, oracle_lib, ids, P4096, slab_bytes=6 * k)
    assert w.log[0]["rows"] == k and w.log[1]["rows"] == k
    check(gpu_ctx, oracle_lib, ids, P4096, slab_bytes=6 * k, window_rows=65)


def test_runs(gpu_ctx, oracle_lib):
    n = 600
    contiguous = np.stack([np.arange(n, dtype=np.uint64) * 10, np.full(n, 10, np.uint64)], axis=1)
    ids = text(list(range(1, n + 1)), width=5)
    # one run open across every slab: nothing is emitted until the last call
    w = check(gpu_ctx, oracle_lib, ids, contiguous, slab_bytes=60)
    assert [e["runs"] for e in w.log[:-1]] == [0] * (len(w.log) - 1) and w.log[-1]["runs"] == 1
    # a run that ends exactly at a cut (row 10 breaks: the 11th id heads the second slab), a run of one id
    broken = contiguous.copy()
    broken[10:, 0] += 5
    broken[20, 0] += 3
    broken[21:, 0] += 9
    w = check(gpu_ctx, oracle_lib, ids, broken, slab_bytes=60)
    assert w.log[1]["runs"] == 1 and w.nruns == 4
    check(gpu_ctx, oracle_lib, ids, broken, slab_bytes=60, window_rows=3)
    # all row lengths 0: no final run (subset.go:285-291), whether the rows abut or not
    zeros = contiguous.copy()
    zeros[:, 1] = 0
    w = check(gpu_ctx, oracle_lib, ids, zeros, slab_bytes=60)
    same = zeros.copy()
    same[:, 0] = 5
    w = check(gpu_ctx, oracle_lib, ids, same, slab_bytes=60)
    assert w.nruns == 0 and w.size == 0
    check(gpu_ctx, oracle_lib, text(SPARSE), parent_table(4096, seed=9, zero=True), slab_bytes=1000, window_rows=64)


BASE = list(range(3, 3000, 7))  # 429 ids, 6-byte lines: 2574 bytes
BAD = {
    "syntax": lambda ids, k: b"12x45\n",
    "range": lambda ids, k: b"99999999999999999999\n",
    "sort": lambda ids, k: b"%05d\n" % (ids[k - 1] - 1 if k else 0),
    "equal": lambda ids, k: b"%05d\n" % (ids[k - 1] if k else 0),
    "exist": lambda ids, k: b"03500\n",   # above ilength 3400
    "read": lambda ids, k: b"03300\n",    # above the 3200 parent rows, below ilength
}


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("window", [0, 3])
def test_errors(gpu_ctx, oracle_lib, kind, window):
    """each error in the first, a middle and the last slab and at the first line of a slab (600-byte
    slabs hold 100 lines): Go's text, the totals and the tables at the error, EINVAL afterwards"""
    par = parent_table(3200, seed=11)
    for k in (0, 5, 100, 250, 400, 428):
        lines = [b"%05d\n" % i for i in BASE]
        lines[k] = BAD[kind](BASE, k)
        ids = b"".join(lines)
        w = check(gpu_ctx, oracle_lib, ids, par, 3400, slab_bytes=600, window_rows=window, after_error=1)
        assert w.outcome == "err" and w.log[-1]["status"] == EINVAL and w.log[-2]["status"] == EFORMAT
        if kind in ("sort", "equal") and k:
            assert w.err.endswith(b"after value %d" % BASE[k - 1])  # (k = 100, 400: the carried id)
        if window == 3 and k > 5:  # the stops before the error line are reported first
            assert any(e["stop"] == 2 for e in w.log[:-2])


def test_ilength_below_and_above_parent_count(gpu_ctx, oracle_lib):
    par = parent_table(64, seed=13)
    ids = text([1, 5, 30, 50, 60, 64, 65, 70])
    for il in (40, 64, 66, 100):
        for slab in (8, 1 << 20):
            check(gpu_ctx, oracle_lib, ids, par, il, slab_bytes=slab, window_rows=8)


def test_espace_leaves_the_carry(gpu_ctx, oracle_lib):
    """tables too short for a call: ESPACE with what it needs, the repeated call goes on as if
    nothing had happened"""
    ids = text(SPARSE, blank_every=9)
    w = check(gpu_ctx, oracle_lib, ids, P4096, slab_bytes=1000, rows_cap=1, runs_cap=64)
    assert any(e["status"] == ESPACE for e in w.log)
    w = check(gpu_ctx, oracle_lib, ids, P4096, slab_bytes=1000, rows_cap=1000, runs_cap=0)
    assert any(e["status"] == ESPACE for e in w.log)
    w = check(gpu_ctx, oracle_lib, ids, P4096, slab_bytes=1000, window_rows=64, rows_cap=0, runs_cap=0)
    assert sum(e["status"] == ESPACE for e in w.log) >= 2


@pytest.mark.parametrize("slab", [64, 1024, 1 << 20])
def test_without_runs(gpu_ctx, oracle_lib, slab):
    for ids, il in ((text(SPARSE, blank_every=4), None), (text(SPARSE) + b"77\n", None), (text(DENSE), 1000)):
        rows, count, size, err = oracle_lib.create_subset_index(ids, P4096, il)
        w = subslab.walk(gpu_ctx, ids, P4096, il, slab_bytes=slab, window_rows=65, want_runs=False)
        assert w.err == err and len(w.runs) == 0 and w.nruns == 0
        if err is None:
            assert np.array_equal(w.rows, rows) and (w.count, w.size) == (count, size)


def test_line_longer_than_a_slot(gpu_ctx, oracle_lib):
    """a 200 KB line of zeros ending in 7 under a 64 KiB halo: stop 1 while it does not head the slab,
    then no slot can hold it; a slot that does hold it parses it like Go"""
    par = parent_table(16, seed=17)
    ids = b"1\n2\n" + b"0" * 200000 + b"7\n9\n"
    w = subslab.walk(gpu_ctx, ids, par, slab_bytes=4096, halo=65536)
    assert w.outcome == "nomem"
    assert (w.log[0]["stop"], w.log[0]["next_off"], w.log[0]["rows"]) == (1, 4, 2)
    assert (w.log[1]["lo"], w.log[1]["stop"], w.log[1]["next_off"]) == (4, 1, 4)
    w = check(gpu_ctx, oracle_lib, ids, par, slab_bytes=1 << 18, halo=65536)
    assert w.count == 4


def test_empty_and_blank_texts(gpu_ctx, oracle_lib):
    par = parent_table(8, seed=19)
    for ids in (b"", b"\n", b"\n\n\n\n", b"5", b"\n5"):
        check(gpu_ctx, oracle_lib, ids, par, slab_bytes=2, halo=1)


def test_carry_refuses_what_would_lose_a_line(gpu_ctx, oracle_lib):
    """a first slab submitted again once the walk is past it (an abandoned walk's carry, not zeroed)
    and a slab that starts past the next unconsumed line are EINVAL; the slab in order goes on, and
    a zeroed carry starts a new walk"""
    from shock_amd import _lib as L
    par = parent_table(16, seed=21)
    ids = b"1\n2\n3\n5\n"
    rows, runs, size, err = oracle_lib.subset(ids, par)
    slot, pslot = gpu_ctx.alloc(64), gpu_ctx.alloc(16 * 16)
    pslot.upload(par.tobytes())
    d_rows, d_runs, carry = gpu_ctx.alloc(16 * 8), gpu_ctx.alloc(16 * 8), gpu_ctx.subset_carry()

    def call(lo, n):
        front = min(lo, 16)
        slot.fill(0xEE)
        slot.upload(ids[lo - front:], 16 - front)
        s = L.Slab(d_data=slot.ptr + 16, n=n, end=len(ids) - lo, front=front, base=lo, is_first=int(lo == 0),
                   is_last=int(lo + n == len(ids)), seq=0, reserved=0)
        return gpu_ctx.subset_slab(s, len(ids), pslot.ptr, 0, 16, 16, 16, True, carry.ptr, d_rows.ptr, 8, d_runs.ptr, 8)

    try:
        r = call(0, 4)
        assert (r.status, r.stop, r.rows, r.next_off) == (0, 0, 2, 4)
        assert call(0, 4).status == EINVAL          # the walk is past the first slab
        assert call(6, 2).status == EINVAL          # the line at 4 would belong to no slab
        r = call(4, 4)                              # the refusals left the carry as it was
        assert (r.status, r.stop, r.count, r.nruns, r.size) == (0, 0, len(rows), len(runs), size)
        assert call(0, 4).status == EINVAL          # the walk is over
        carry.upload(bytes(carry.nbytes))           # zeroed: a new walk
        r = call(0, 4)
        assert (r.status, r.rows, r.count) == (0, 2, 2) and np.array_equal(d_rows.rows(2), rows[:2])
    finally:
        for b in (slot, pslot, d_rows, d_runs, carry):
            b.free()


def test_espace_names_the_final_run(gpu_ctx, oracle_lib):
    """rows too short on the last slab: the runs asked for count the final run (oSize is summed from
    the parent window, not from the short table), so one repeat is enough"""
    par = parent_table(64, seed=23)
    ids = text([3, 4, 9, 10, 11, 40])
    rows, runs, size, err = oracle_lib.subset(ids, par)
    w = check(gpu_ctx, oracle_lib, ids, par, rows_cap=1, runs_cap=0)
    sp = [e for e in w.log if e["status"] == ESPACE]
    assert len(sp) == 1 and (sp[0]["rows"], sp[0]["runs"]) == (len(rows), len(runs)) and size > 0
