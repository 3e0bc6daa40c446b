"""A driver for the column index's slab pass: walks a file's bytes through Context.column_slab by
the protocol of include/shockidx.h (slabs in file order, one carry on the device, the retry rule
of sidx_colwalk.hpp).  Test support only.

Each slab's window -- `front` bytes before it, the slab, its halo -- is uploaded into a slot of
exactly that size plus padding, so a read outside the window does not find the file's bytes.

walk(...) returns (outcome, rows, log):
    ("ok", rows)      rows: uint64 [k, 2], the slabs' rows concatenated
    ("err", None)     a slab returned EFORMAT (the rows of earlier slabs are dropped)
    ("nomem", None)   EMORE for the line that heads a slab: no slot can hold it
log: one (lo, n, status, count_or_state_out) per call made.
"""
import numpy as np

FRONT = 16


def slab_at(lo, S, halo, size):
    n = min(S, size - lo)
    end = min(n + halo, size - lo)
    return lo, n, end


def walk(ctx, data: bytes, column: int, slab_bytes: int, halo: int, row_cap: int | None = None, max_calls: int = 100000):
    from shock_amd import _lib as L
    size = len(data)
    halo = min(halo, size)
    carry = ctx.column_carry()
    slot = ctx.alloc(FRONT + slab_bytes + halo + 64)
    cap = row_cap if row_cap is not None else slab_bytes // 32 + 64
    d_rows = ctx.alloc(16 * max(cap, 1))
    out, log = [], []
    try:
        lo, n, end = slab_at(0, max(slab_bytes, 1), halo, size)
        while True:
            front = FRONT if lo >= FRONT else 0
            slot.fill(0xEE)  # (what lies outside the window is not the file)
            slot.upload(data[lo - front:lo + end], FRONT - front)
            while True:
                assert len(log) < max_calls
                s = L.Slab(d_data=slot.ptr + FRONT, n=n, end=end, front=front, base=lo, is_first=int(lo == 0),
                           is_last=int(lo + n == size), seq=0, reserved=0)
                r = ctx.column_slab(s, size, column, carry.ptr, d_rows.ptr, cap)
                log.append((lo, n, r.status, r.state_out if r.status == L.EMORE else r.count))
                if r.status == L.ESPACE:
                    cap = r.count
                    d_rows.free()
                    d_rows = ctx.alloc(16 * cap)
                    continue
                if r.status == L.EMORE:
                    x = r.state_out
                    assert (x == 0 and lo == 0) or lo < x <= lo + n, (lo, n, x)  # an owned line: after a '\n' of the slab
                    if x == 0 or x - 1 <= lo:
                        return "nomem", None, log
                    n = x - 1 - lo  # shortened: the slab no longer owns the line
                    end = min(n + halo, size - lo)
                    continue
                break
            if r.status == L.EFORMAT:
                assert r.count == 0 and r.err is not None
                return "err", r.err, log
            assert r.status == L.OK, (r.status, r.err)
            if r.count:
                out.append(d_rows.rows(r.count))
            if lo + n == size:
                break
            lo, n, end = slab_at(lo + n, slab_bytes, halo, size)
        rows = np.concatenate(out) if out else np.zeros((0, 2), np.uint64)
        return "ok", rows, log
    finally:
        carry.free()
        slot.free()
        d_rows.free()
