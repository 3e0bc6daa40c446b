"""A driver for the subset indexes' slab pass: walks an id text and a parent index through
Context.subset_slab by the protocol of include/shockidx.h (id slabs in file order, one carry on the
device, the parent index window by window, the decisions of sidx_subwalk.hpp).  Test support only.

Each id slab's window -- `front` bytes before it, the slab, its halo -- and each parent window are
uploaded into slots of exactly their size, filled with 0xEE around them, so a read outside a
window does not find the file's bytes.

walk(...) returns a Walk:
    outcome   "ok", "err" (a call returned EFORMAT: err holds Go's text), "nomem" (stop 1 for the
              line that heads a slab: no slot can hold it) or "einval"
    rows, runs   uint64 [k, 2]: the calls' tables concatenated
    count, nruns, size   the last call's running totals
    log       one dict per call: lo, n, prow0, prows, status, stop, next_off, next_id, rows, runs
"""
from dataclasses import dataclass, field

import numpy as np

FRONT = 16
PAD = 64


@dataclass
class Walk:
    outcome: str = "ok"
    rows: np.ndarray | None = None
    runs: np.ndarray | None = None
    count: int = 0
    nruns: int = 0
    size: int = 0
    err: bytes | None = None
    log: list = field(default_factory=list)


def walk(ctx, ids: bytes, parent, ilength=None, slab_bytes: int = 1 << 20, halo: int = 65536, window_rows: int = 0,
         want_runs: bool = True, rows_cap: int | None = None, runs_cap: int | None = None, after_error: int = 0,
         max_calls: int = 100000) -> Walk:
    """rows_cap / runs_cap: the tables the first call gets (ESPACE grows them to what the call asks
    for and repeats it).  after_error: calls to make after an EFORMAT (each must be EINVAL)."""
    from shock_amd import _lib as L
    par = np.ascontiguousarray(parent, dtype=np.uint64).reshape(-1, 2)
    pc = par.shape[0]
    il = pc if ilength is None else int(ilength)
    size = len(ids)
    halo = min(halo, size)
    slab_bytes = max(min(slab_bytes, size), 1)
    W = window_rows if window_rows else max(pc, 1)
    carry = ctx.subset_carry()
    slot = ctx.alloc(FRONT + slab_bytes + halo + PAD)
    pslot = ctx.alloc(16 * (W + 2))
    rcap = rows_cap if rows_cap is not None else slab_bytes // 2 + 2
    ucap = runs_cap if runs_cap is not None else slab_bytes // 2 + 3
    d_rows, d_runs = ctx.alloc(16 * max(rcap, 1)), ctx.alloc(16 * max(ucap, 1))
    w = Walk()
    rows, runs = [], []

    def window(row0):
        row0 = min(row0, pc)
        k = min(W, pc - row0)
        pslot.fill(0xEE)
        if k:
            pslot.upload(par[row0:row0 + k].tobytes(), 16)
        return row0, k

    try:
        prow0, prows = window(0)
        lo = 0
        while True:
            n = min(slab_bytes, size - lo)
            end = min(n + halo, size - lo)
            front = FRONT if lo >= FRONT else lo
            slot.fill(0xEE)  # (what lies outside the window is not the file)
            if end + front:
                slot.upload(ids[lo - front:lo + end], FRONT - front)
            while True:
                assert len(w.log) < max_calls
                s = L.Slab(d_data=slot.ptr + FRONT, n=n, end=end, front=front, base=lo, is_first=int(lo == 0),
                           is_last=int(lo + n == size), seq=0, reserved=0)
                r = ctx.subset_slab(s, size, pslot.ptr + 16, prow0, prows, pc, il, want_runs, carry.ptr, d_rows.ptr, rcap,
                                    d_runs.ptr, ucap)
                w.log.append(dict(lo=lo, n=n, prow0=prow0, prows=prows, status=r.status, stop=r.stop,
                                  next_off=int(r.next_off), next_id=int(r.next_id), rows=int(r.rows), runs=int(r.runs)))
                if r.status == L.ESPACE:
                    if r.rows > rcap:
                        rcap = int(r.rows)
                        d_rows.free()
                        d_rows = ctx.alloc(16 * rcap)
                    if r.runs > ucap:
                        ucap = int(r.runs)
                        d_runs.free()
                        d_runs = ctx.alloc(16 * ucap)
                    continue
                if r.status == L.EINVAL:
                    w.outcome = "einval"
                    return w
                if r.rows:
                    rows.append(d_rows.rows(int(r.rows)).copy())
                if r.runs:
                    runs.append(d_runs.rows(int(r.runs)).copy())
                w.count, w.nruns, w.size = int(r.count), int(r.nruns), int(r.size)
                if r.status == L.EFORMAT:
                    w.outcome, w.err = "err", r.message
                    for _ in range(after_error):
                        r2 = ctx.subset_slab(s, size, pslot.ptr + 16, prow0, prows, pc, il, want_runs, carry.ptr,
                                             d_rows.ptr, rcap, d_runs.ptr, ucap)
                        w.log.append(dict(lo=lo, n=n, prow0=prow0, prows=prows, status=r2.status, stop=r2.stop,
                                          next_off=0, next_id=0, rows=0, runs=0))
                    return w
                assert r.status == L.OK
                if r.stop == 2:  # the same slab against the window that starts at the id's row
                    assert 1 <= r.next_id <= pc and lo <= r.next_off < lo + n
                    prow0, prows = window(int(r.next_id) - 1)
                    continue
                break
            if r.stop == 1:
                assert lo <= r.next_off < lo + n
                if r.next_off <= lo:
                    w.outcome = "nomem"
                    return w
                lo = int(r.next_off)  # every line before it is consumed: a fresh slot from the open line on
                continue
            lo += n
            if lo >= size:
                return w
    finally:
        z = np.zeros((0, 2), np.uint64)
        w.rows = np.concatenate(rows) if rows else z
        w.runs = np.concatenate(runs) if runs else z
        for b in (carry, slot, pslot, d_rows, d_runs):
            b.free()
