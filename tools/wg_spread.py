"""How unequal the workgroups of k_fq_tiles finish (dev tool; needs the SIDX_DIAG variant:
`make -C shock_amd/csrc variant V=diag VFLAGS=-DSIDX_DIAG=1`, run with SHOCKIDX_VARIANT=diag).

usage: SHOCKIDX_VARIANT=diag python tools/wg_spread.py [size_gib] [out.json]
Each workgroup's wave 0 sums the s_memtime ticks of every phase of every tile it ran and counts
its tiles; the kernel ends with the workgroup whose sum is largest.  Prints (and writes) one JSON
object: the distribution over workgroups of the tick sums -- min, median, p99, max and
(max - mean) / max, the share of the kernel that perfectly even finish times would save -- for all
workgroups and split by the number of tiles a workgroup ran."""
import ctypes
import json
import os
import sys

import numpy as np

os.environ["SHOCKIDX_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shock_amd import Context, _lib  # noqa: E402
from shock_amd.synth import SynthFile  # noqa: E402


def dist(x):
    x = np.asarray(x, dtype=np.float64)
    return {"n": int(x.size), "min": float(x.min()), "median": float(np.median(x)),
            "p99": float(np.percentile(x, 99)), "max": float(x.max()), "mean": round(float(x.mean()), 1),
            "max_minus_mean_over_max": round(float((x.max() - x.mean()) / x.max()), 4)}


size = int(float(sys.argv[1]) * (1 << 30)) if len(sys.argv) > 1 else 10 << 30
ctx = Context(0)
sf = SynthFile(ctx, "fastq", size)
data = sf.window(0, size)
rows = ctx.alloc(16 * (sf.expected_count() + 1024))
for _ in range(5):
    r = ctx.build_buffer(data, size, rows, kind="record", fmt="fastq")
L = _lib.lib()
L.shockidx_debug_tiles_grid.restype = ctypes.c_int
L.shockidx_debug_tiles_grid.argtypes = [ctypes.c_void_p]
nwg = L.shockidx_debug_tiles_grid(ctx._h)
out = np.zeros(9 * 2 * nwg, dtype=np.uint64)
L.shockidx_debug_timing(ctx._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(2 * nwg))
t = out.reshape(nwg, 2, 9)
tot = t[:, 0, :6].sum(axis=1).astype(np.float64)  # wave 0: the certifying wave, every phase of every tile
ntl = t[:, 0, 8].astype(np.int64)
res = {"bytes": size, "grid": int(nwg), "index_ms": round(float(r.timings["index_ms"]), 4), "ok": bool(r.ok),
       "count": int(r.count), "unit": "s_memtime ticks, summed over a workgroup's tiles (wave 0)",
       "tiles_per_wg": {"min": int(ntl.min()), "median": float(np.median(ntl)), "max": int(ntl.max())},
       "all": dist(tot), "by_tiles": {}}
vals, cnts = np.unique(ntl, return_counts=True)
if len(vals) <= 8:
    for v in vals:
        res["by_tiles"][str(int(v))] = dist(tot[ntl == v])
else:  # dynamic claims: the counts spread out; the quartiles of the tile count instead
    q = np.percentile(ntl, [25, 50, 75])
    edges = [ntl.min() - 1, q[0], q[1], q[2], ntl.max()]
    for i in range(4):
        m = (ntl > edges[i]) & (ntl <= edges[i + 1])
        if m.any():
            res["by_tiles"][f"{int(edges[i]) + 1}-{int(edges[i + 1])}"] = dist(tot[m])
res["ticks_per_tile"] = round(float(tot.sum() / ntl.sum()), 1)
s = json.dumps(res)
print(s)
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        f.write(s + "\n")
