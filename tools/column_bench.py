"""Column index build timing on the device: the tile pass vs the general build
(SHOCKIDX_COLUMN_MODE=two) at columns 1 and 12, next to the line index of the same buffer in the
same process.  The body is one generated block of 12-column similarity-like rows (about 100
bytes each, runs of 1-50 rows per column-1 key) repeated to --mib MiB in HBM; the expected table
is derived with numpy from tests/colref.py's table of the block (block cuts shifted by multiples
of the block size, plus a cut at each block seam iff the seam keys differ).
Prints one JSON line.  Dev tool; the GPU tests carry the parity cases."""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=6144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--block-mib", type=int, default=8)
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
