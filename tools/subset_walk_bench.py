"""The subset indexes' slab walk against the whole build, in one process, over files of a size that
fits both paths:
  whole   Context.subset_host: the id text and the parent rows uploaded whole, one
          shockidx_subset_index, both tables downloaded
  walk    shockidx_subset_fd_walk with explicit sizes (--slab id bytes, --window parent rows)
  capped  shockidx_subset_create on a context capped at --cap bytes, which takes the walk by itself
          (asserted from its stats) and writes and renames both .idx files
for a dense id list (every row) and a 1 % list over --rows parent rows.  The tables of the three arms
are checked to be equal.  Times are medians of the call's wall time over --steps calls after 2
warm-up calls (file reads come out of the page cache); held is the device bytes the context's
caches held when the walk ended.  The arms are whole calls, not kernel for kernel: `whole` allocates,
uploads and downloads through Python on every call, `walk` reuses the context's buffers and returns
tables, `capped` also writes two files.  Prints one JSON line.  Dev tool; tests/test_gpu_subset_walk.py
carries the parity cases."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shock_amd import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--slab", type=int, default=4 << 20)
    ap.add_argument("--window", type=int, default=1 << 20)
    ap.add_argument("--cap", type=int, default=64 << 20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    lens = rng.integers(50, 400, a.rows).astype(np.uint64)
    gaps = (rng.random(a.rows) < 0.05).astype(np.uint64) * 3
    par = np.stack([np.cumsum(lens + gaps) - lens, lens], axis=1)
    out = {"metric": "subset indexes: slab walk over files vs whole build", "unit": "ms", "steps": a.steps, "warmup": 2,
           "parent_rows": a.rows, "slab_bytes": a.slab, "window_rows": a.window, "cap_bytes": a.cap,
           "build": "hipcc -O3 --offload-arch=gfx950", "lists": {}}

    def timed(fn):
        for _ in range(2):
            r = fn()
        ws = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            r = fn()
            ws.append((time.perf_counter() - t0) * 1e3)
        return r, {"call_ms": round(float(np.median(ws)), 3), "call_min": round(min(ws), 3), "call_max": round(max(ws), 3)}

    with tempfile.TemporaryDirectory() as td:
        pp = os.path.join(td, "parent.idx")
        par.astype("<u8").tofile(pp)
        fp = os.open(pp, os.O_RDONLY)
        for name, picks in (("dense", np.arange(1, a.rows + 1)), ("one_percent", np.flatnonzero(rng.random(a.rows) < 0.01) + 1)):
            ids = b"".join(b"%d\n" % i for i in picks.tolist())
            pi = os.path.join(td, name + ".txt")
            with open(pi, "wb") as f:
                f.write(ids)
            fi = os.open(pi, os.O_RDONLY)
            res = {"ids": int(len(picks)), "ids_bytes": len(ids)}
            ctx = Context(0)
            whole, res["whole"] = timed(lambda: ctx.subset_host(ids, par, a.rows))
            res["whole"]["held"] = ctx.workspace_bytes()
            walk, res["walk"] = timed(lambda: ctx.subset_fd_walk(fi, len(ids), fp, par.nbytes, a.rows, True, a.slab, a.window))
            res["walk"].update(ctx.subset_stats())
            ctx.close()
            ctx = Context(0)
            ctx.set_dev_cap(a.cap)
            co, o = os.path.join(td, name + ".subset.idx"), os.path.join(td, name + ".idx")
            capped, res["capped"] = timed(lambda: ctx.subset_create(fi, len(ids), fp, par.nbytes, a.rows, td, co, o))
            res["capped"].update(ctx.subset_stats())
            assert res["capped"]["walked"] == 1 and res["capped"]["held_bytes"] <= a.cap
            ctx.close()
            capped.rows = np.fromfile(o, dtype="<u8").reshape(-1, 2)
            capped.run_rows = np.fromfile(co, dtype="<u8").reshape(-1, 2)
            for r in (walk, capped):
                assert whole.ok and r.ok and (r.count, r.runs, r.size) == (whole.count, whole.runs, whole.size)
                assert np.array_equal(r.rows, whole.rows) and np.array_equal(r.run_rows, whole.run_rows)
            res["tables_equal"] = True
            res["walk_over_whole"] = round(res["walk"]["call_ms"] / res["whole"]["call_ms"], 3)
            res["capped_over_whole"] = round(res["capped"]["call_ms"] / res["whole"]["call_ms"], 3)
            out["lists"][name] = res
            os.close(fi)
        os.close(fp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
