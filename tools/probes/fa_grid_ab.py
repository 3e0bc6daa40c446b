"""FASTA 10 GiB: the product library with the tile grid at its own size (8 per CU) against a context
capped to 7 workgroups per CU (shockidx_debug_set_tiles_grid), two contexts of each, taking turns in
one process on one input (dev tool, runs on the GPU box; DESIGN.md §3 "Registers of the tile loop").

  python tools/probes/fa_grid_ab.py [CUs, default 256] > profiles/spills/ab_fasta_grid7.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from shock_amd import Context  # noqa: E402
from shock_amd.synth import SynthFile  # noqa: E402

cus = int(sys.argv[1]) if len(sys.argv) > 1 else 256
size = 10 << 30
gen = Context(0)
sf = SynthFile(gen, "fasta", size)
data = sf.window(0, size)
arms = {}
for name, g in (("own", 0), ("cap7", 7 * cus), ("own_b", 0), ("cap7_b", 7 * cus)):
    ctx = Context(0)
    if g:
        ctx.debug_set_tiles_grid(g)
    rows = ctx.alloc(16 * (sf.expected_count() + 1024))
    arms[name] = (ctx, rows, [], [])
for name, (ctx, rows, k, b) in arms.items():
    for _ in range(20):
        ctx.build_buffer(data, size, rows, kind="record", fmt="fasta")
for rnd in range(6):
    order = list(arms) if rnd % 2 == 0 else list(arms)[::-1]
    for name in order:
        ctx, rows, k, b = arms[name]
        for _ in range(10):
            r = ctx.build_buffer(data, size, rows, kind="record", fmt="fasta")
            assert r.ok and r.count == sf.expected_count()
            k.append(r.timings["index_ms"])
            b.append(r.timings["kernel_ms"])
    print(f"round {rnd + 1}", file=sys.stderr, flush=True)
print(json.dumps({"fmt": "fasta", "bytes": size, "cus": cus,
                  "arms": {n: {"grid": "8 per CU (occupancy)" if "own" in n else f"{7 * cus} (7 per CU)",
                               "k_med": round(float(np.median(k)), 4), "b_med": round(float(np.median(b)), 4), "n": len(k)}
                           for n, (_, _, k, b) in arms.items()}}))
