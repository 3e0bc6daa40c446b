"""The download plan on the device next to the loop the library offered before it, measured in the
same process and alternating:
  plan      one shockidx_download_plan call for all parts, the sections left in HBM
  per_part  one shockidx_idx_range call per part (the records left on the device, then copied back),
            the joined list uploaded again for the stream; for CHUNK_RANGE one more idx_range per
            matrix record, as controller/node/single.go:403-425 composes them
over a record table of 2^20 rows in which every 7th pair is not contiguous.  RANGE: P parts of
2^20 / P rows each, P = 1, 16, 256, 4096 (the same rows visited in total).  CHUNK_RANGE: 64 parts, one
matrix row each, over the table's chunkrecord matrix index.  Both sides are checked to give the same
sections before anything is timed.  Times are medians over --steps calls after --warmup calls;
call_ms is the wall time of the Python call(s), every host wait included, device_ms the plan's own
HIP-event time.  Writes the JSON to --out and prints it.  Dev tool; the GPU tests carry the parity
cases."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shock_amd import Context  # noqa: E402
from shock_amd import _lib as L  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan", "bench_plan.json"))
    a = ap.parse_args()
    n = a.rows
    ctx = Context(0)
    ln = np.full(n, 100, dtype=np.uint64)
    gap = np.where(np.arange(n) % 7 == 0, 3, 0).astype(np.uint64)  # the pair (i - 1, i) is not contiguous
    pos = np.cumsum(ln + gap) - ln
    tab = np.ascontiguousarray(np.stack([pos, ln], axis=1))
    d_rows = ctx.alloc(16 * n + 64)
    d_rows.upload(tab.tobytes())
    d_secs, d_tmp, d_up = ctx.alloc(16 * n + 64), ctx.alloc(16 * n + 64), ctx.alloc(16 * n + 64)
    out = {"metric": "download plan: all parts of an index download, device-resident index", "rows": n, "unit": "ms",
           "steps": a.steps, "warmup": a.warmup, "build": "hipcc -O3 --offload-arch=gfx950"}

    def plan_range(parts):
        return ctx.download_plan(L.PLAN_RANGE, parts, d_rows.ptr, n, n, d_secs=d_secs.ptr, secs_cap=n)

    def loop_range(parts):
        got = []
        for p in parts:
            k, err = ctx.idx_range(d_rows.ptr, n, p, n, d_tmp.ptr, n)
            assert err is None
            if k:
                got.append(d_tmp.rows(k))
        secs = np.concatenate(got) if got else np.zeros((0, 2), np.uint64)
        if len(secs):
            d_up.upload(secs.tobytes())
        return secs

    def alternate(fa, fb):
        for _ in range(a.warmup):
            fa()
            fb()
        ta, tb, dev = [], [], []
        for _ in range(a.steps):
            t = time.perf_counter()
            r = fa()
            ta.append((time.perf_counter() - t) * 1e3)
            dev.append(r.kernel_ms)
            t = time.perf_counter()
            fb()
            tb.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ta)), float(np.median(dev)), float(np.median(tb))

    rng = {}
    for P in (1, 16, 256, 4096):
        per = n // P
        parts = [f"{i * per + 1}-{(i + 1) * per}" for i in range(P)]
        r = plan_range(parts)
        assert r.ok, (r.status, r.err)
        ref = loop_range(parts)
        assert r.count == len(ref) and np.array_equal(d_secs.rows(r.count), ref)
        pm, dm, lm = alternate(lambda: plan_range(parts), lambda: loop_range(parts))
        rng[str(P)] = {"parts": P, "rows_per_part": per, "sections": r.count, "plan_call_ms": round(pm, 4),
                       "plan_device_ms": round(dm, 4), "per_part_call_ms": round(lm, 4), "per_part_over_plan": round(lm / pm, 2)}
    out["range"] = rng

    # CHUNK_RANGE: the table as a subset node's record index, its matrix index, 64 single-row parts
    m = ctx.chunkrecord_subset(tab)
    assert m.ok and m.count >= 64, m.count
    mat, M = m.rows, m.count
    d_mat = ctx.alloc(16 * M + 64)
    d_mat.upload(mat.tobytes())
    parts = [str(1 + (i * (M // 64))) for i in range(64)]

    def plan_chunk():
        return ctx.download_plan(L.PLAN_CHUNK_RANGE, parts, d_mat.ptr, M, M, d_rows.ptr, n, n, d_secs=d_secs.ptr, secs_cap=n)

    def loop_chunk():
        got = []
        for p in parts:
            crecs, err = ctx.idx_range(d_mat.ptr, M, p, M)
            assert err is None
            for c0, c1 in crecs.tolist():
                start = c0 // 16 + 1
                stop = start - 1 + c1 // 16
                k, err = ctx.idx_range(d_rows.ptr, n, f"{start}-{stop}", n, d_tmp.ptr, n)
                assert err is None
                if k:
                    got.append(d_tmp.rows(k))
        secs = np.concatenate(got)
        d_up.upload(secs.tobytes())
        return secs

    r = plan_chunk()
    assert r.ok, (r.status, r.err)
    ref = loop_chunk()
    assert r.count == len(ref) and np.array_equal(d_secs.rows(r.count), ref)
    pm, dm, lm = alternate(plan_chunk, loop_chunk)
    out["chunk_range"] = {"parts": 64, "matrix_rows": M, "sections": r.count, "plan_call_ms": round(pm, 4),
                          "plan_device_ms": round(dm, 4), "per_part_call_ms": round(lm, 4),
                          "per_part_over_plan": round(lm / pm, 2)}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
