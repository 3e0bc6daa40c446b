"""Column index build timing on the device: the tile pass vs the general build
(SHOCKIDX_COLUMN_MODE=two) at columns 1 and 12, next to the line index of the same buffer in the
same process.  The body is one generated block of 12-column similarity-like rows (about 100
bytes each, runs of 1-50 rows per column-1 key) repeated to --mib MiB in HBM; the expected table
is derived with numpy from tests/colref.py's table of the block (block cuts shifted by multiples
of the block size, plus a cut at each block seam iff the seam keys differ).
Prints one JSON line.  Dev tool; the GPU tests carry the parity cases.

--slabs: instead, in one process over the same resident input, the whole tile-pass build (the
control) and the slab pass (Context.column_slab, slab after slab with the carry on the device) at
1 GiB and at 64 MiB slabs with a 4 MiB halo, columns 1 and 12: the median over --steps builds of
the summed device time and of the wall time, 3 warm-up builds each; the tables are hashed and must
all be equal.  --e2e-gib G adds Context.column_create over a page-cached G GiB file, once without a
device cap and once under --e2e-cap-mib: GiB/s and the device bytes the context held."""
import argparse
import hashlib
import json
import tempfile
import time
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import colref  # noqa: E402
from shock_amd import Context  # noqa: E402

PEAK = 8e12  # bytes/s


def make_block(seed: int, nbytes: int) -> bytes:
    """BLAST-m8-like rows: query, subject, identity, length, mismatches, gaps, 4 coordinates,
    e-value, bit score; the query (column 1) in runs of 1-50 rows."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    q = 0
    while len(out) < nbytes:
        q += 1
        query = b"mgm%07d_%d_%d_+" % (q, int(rng.integers(1, 5000)), int(rng.integers(5000, 9999)))
        for _ in range(int(rng.integers(1, 51))):
            v = rng.integers(1, 100000, 9)
            out += b"%s\tgi|%d|ref|WP_%09d.1|\t%.2f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.1e\t%.1f\n" % (
                query, v[0] * 37, v[1] * 911, 50 + (v[2] % 5000) / 100.0, v[3] % 400 + 30, v[4] % 60, v[5] % 8,
                v[6] % 900 + 1, v[6] % 900 + 200, v[7] % 900 + 1, v[7] % 900 + 200, 10.0 ** -(v[8] % 80),
                40 + (v[8] % 3000) / 10.0)
    return bytes(out)


def expected_rows(block: bytes, column: int, reps: int) -> np.ndarray:
    st = colref.column_index(block, column)
    assert st[0] == "ok", st
    bs = len(block)
    cuts = np.array([o for o, _ in st[1][1:]], dtype=np.uint64)
    lines = block.split(b"\n")[:-1]
    first, last = ((ln + b"\n").split(b"\t")[column - 1] for ln in (lines[0], lines[-1]))
    later = np.concatenate([np.zeros(1, np.uint64), cuts]) if first != last else cuts
    base = (np.arange(1, reps, dtype=np.uint64) * np.uint64(bs))[:, None]
    allc = np.concatenate([cuts, (base + later[None, :]).reshape(-1)])
    if allc.size == 0:
        return np.zeros((0, 2), np.uint64)
    pts = np.concatenate([np.zeros(1, np.uint64), allc, np.array([bs * reps], np.uint64)])
    return np.stack([pts[:-1], pts[1:] - pts[:-1]], axis=1)


def slab_build(ctx, L, data, n, column, S, halo, carry, rows, row_cap):
    """One build through column_slab: (rows, summed device ms, slabs)."""
    total, dev, k, lo = 0, 0.0, 0, 0
    while lo < n:
        m = min(S, n - lo)
        s = L.Slab(d_data=data.ptr + lo, n=m, end=min(m + halo, n - lo), front=lo, base=lo, is_first=int(lo == 0),
                   is_last=int(lo + m == n), seq=0, reserved=0)
        r = ctx.column_slab(s, n, column, carry.ptr, rows.ptr + 16 * total, row_cap - total)
        if r.status != 0:
            raise RuntimeError(f"slab at {lo}: status {r.status} {r.err}")
        total += r.count
        dev += r.timings["kernel_ms"]
        k += 1
        lo += m
    return total, dev, k


def slabs_main(a, ctx, block, data, n, nlines, reps):
    from shock_amd import _lib as L
    rows = ctx.alloc(16 * (nlines + 64))
    carry = ctx.column_carry()
    out = {"metric": "device-resident column index build: whole tile pass vs slab pass", "bytes": n, "lines": nlines,
           "unit": "ms", "steps": a.steps, "warmup": 3, "halo": 4 << 20, "build": "hipcc -O3 --offload-arch=gfx950"}
    ok = True

    def digest(count):
        return hashlib.blake2b(rows.download(16 * count).tobytes(), digest_size=16).hexdigest()

    for column in (1, 12):
        want = expected_rows(block, column, reps)
        want_h = hashlib.blake2b(np.ascontiguousarray(want, dtype="<u8").tobytes(), digest_size=16).hexdigest()
        ks, ws = [], []
        for i in range(3 + a.steps):
            r = ctx.column_buffer(data, n, column, rows)
            if i >= 3:
                ks.append(r.timings["kernel_ms"])
                ws.append(r.timings["total_ms"])
        e = {"path": r.path, "rows": r.count, "device_ms": round(float(np.median(ks)), 4),
             "call_ms": round(float(np.median(ws)), 4), "hash": digest(r.count)}
        e["table_ok"] = e["hash"] == want_h and r.count == len(want)
        ok = ok and e["table_ok"]
        out[f"column{column}_whole"] = e
        for S in (1 << 30, 64 << 20):
            ks, ws = [], []
            for i in range(3 + a.steps):
                t0 = time.perf_counter()
                count, dev, k = slab_build(ctx, L, data, n, column, S, 4 << 20, carry, rows, nlines + 64)
                wall = (time.perf_counter() - t0) * 1e3
                if i >= 3:
                    ks.append(dev)
                    ws.append(wall)
            s = {"path": 5, "slab_bytes": S, "slabs": k, "rows": count, "device_ms": round(float(np.median(ks)), 4),
                 "wall_ms": round(float(np.median(ws)), 4), "hash": digest(count)}
            s["table_ok"] = s["hash"] == want_h and count == len(want)
            s["vs_whole"] = round(s["device_ms"] / e["device_ms"], 3)
            s["per_slab_extra_us"] = round((s["device_ms"] - e["device_ms"]) * 1e3 / k, 1)
            ok = ok and s["table_ok"]
            out[f"column{column}_slabs_{S >> 20}mib"] = s
    rows.free()
    carry.free()
    if a.e2e_gib:
        data.free()
        with tempfile.TemporaryDirectory() as td:
            body = os.path.join(td, "body")
            ereps = max(1, (a.e2e_gib << 30) // len(block))
            with open(body, "wb") as f:
                for _ in range(ereps):
                    f.write(block)
            size = os.path.getsize(body)
            with open(body, "rb") as f:  # (read once: the pages are in the cache)
                while f.read(64 << 20):
                    pass
            want = expected_rows(block, 1, ereps)
            want_b = np.ascontiguousarray(want, dtype="<u8").tobytes()
            os.mkdir(os.path.join(td, "temp"))
            for tag, cap in (("uncapped", 0), ("capped", a.e2e_cap_mib << 20)):
                c2 = Context(0)
                if cap:
                    c2.set_dev_cap(cap)
                best, res = None, None
                for i in range(3):
                    outp = os.path.join(td, f"{tag}.idx")
                    with open(body, "rb") as f:
                        t0 = time.perf_counter()
                        res = c2.column_create(f.fileno(), size, 1, os.path.join(td, "temp"), outp)
                        dt = time.perf_counter() - t0
                    best = dt if best is None or dt < best else best
                same = res.status == 0 and open(outp, "rb").read() == want_b
                ok = ok and same
                out[f"create_{tag}"] = {"bytes": size, "cap": cap, "path": res.path, "rows": res.count, "reruns": res.reruns,
                                        "best_of_3_s": round(best, 4), "gib_s": round(size / best / (1 << 30), 2),
                                        "device_ms": round(res.timings["kernel_ms"], 3),
                                        "workspace_bytes": c2.workspace_bytes(), "table_ok": bool(same)}
                c2.close()
    out["tables_ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=6144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--block-mib", type=int, default=8)
    ap.add_argument("--slabs", action="store_true", help="whole tile pass vs the slab pass at 1 GiB and 64 MiB slabs")
    ap.add_argument("--e2e-gib", type=int, default=0, help="with --slabs: column_create over a page-cached file of this size")
    ap.add_argument("--e2e-cap-mib", type=int, default=1024)
    a = ap.parse_args()
    block = make_block(1, a.block_mib << 20)
    bs = len(block)
    reps = max(1, (a.mib << 20) // bs)
    n = bs * reps
    nlines = block.count(b"\n") * reps
    ctx = Context(0)
    data = ctx.alloc(n + 64, node=True)
    for r in range(reps):
        data.upload(block, r * bs)
    if a.slabs:
        return slabs_main(a, ctx, block, data, n, nlines, reps)
    rows = ctx.alloc(16 * (nlines + 64))
    out = {"metric": "device-resident column index build", "bytes": n, "lines": nlines, "unit": "ms",
           "steps": a.steps, "warmup": 3, "build": "hipcc -O3 --offload-arch=gfx950"}

    def timed(fn):
        for _ in range(3):
            r = fn()
        ks, ws = [], []
        for _ in range(a.steps):
            r = fn()
            ks.append(r.timings["kernel_ms"])
            ws.append(r.timings["total_ms"])
        return r, float(np.median(ks)), float(np.median(ws))

    def entry(r, ms, wall):
        moved = n + 16 * r.count
        return {"path": r.path, "rows": r.count, "device_ms": round(ms, 4), "call_ms": round(wall, 4),
                "gib_s": round(n / (ms * 1e-3) / (1 << 30), 1), "frac_of_8TBs": round(moved / (ms * 1e-3) / PEAK, 4)}

    ok = True
    r, ms, wall = timed(lambda: ctx.build_buffer(data, n, rows, kind="line"))
    out["line"] = entry(r, ms, wall)
    for column in (1, 12):
        want = expected_rows(block, column, reps)
        for mode in ("tiles", "two"):
            if mode == "two":
                os.environ["SHOCKIDX_COLUMN_MODE"] = "two"
            r, ms, wall = timed(lambda: ctx.column_buffer(data, n, column, rows))
            os.environ.pop("SHOCKIDX_COLUMN_MODE", None)
            e = entry(r, ms, wall)
            e["table_ok"] = bool(r.status == 0 and r.count == len(want) and np.array_equal(rows.rows(r.count), want))
            e["vs_line"] = round(ms / out["line"]["device_ms"], 3)
            ok = ok and e["table_ok"]
            out[f"column{column}_{mode}"] = e
    out["tables_ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
