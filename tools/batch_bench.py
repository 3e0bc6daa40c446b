"""The batch build on the device against what the library offered before, in one process:
  batch    shockidx_build_batch_device over K nodes of one size (every node on the batched walk)
  singles  the same call with SHOCKIDX_BATCH_SMALL=0: every node through the single build, one at a
           time (the call's own loop over run_index)
  loop     K shockidx_build_device calls from Python, one per node (the caller's loop)
for node sizes from 4 KiB to 4 MiB -- the A/B behind the small-node limit (SHOCKIDX_BATCH_SMALL) --
for each format at one size, and for short lists (1, 8 and 64 nodes: a wave walks a whole node, so a
short list of long nodes leaves the device idle).  Nodes are whole records of tests-style synthetic text, packed at
16-byte aligned positions of one arena in HBM.  Times are medians over --steps calls after 2 warm-up
calls: call_ms is the call's wall time (its host waits included), device_ms its HIP-event time.
Prints one JSON line.  Dev tool; tests/test_gpu_batch.py carries the parity cases."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shock_amd import Context  # noqa: E402


def _fastq(n):
    rec = b"@read%06d/1\n" + b"ACGTTGCAAGGCTTAACCGGTTAACCGGTTAAGGCCTTAAGGCCAATTGGCCAATTGGCCAATTGGCC" * 2 + b"\n+\n" + b"I" * 136 + b"\n"
    return b"".join(rec % i for i in range(max(n // len(rec % 0), 1)))


def _fasta(n):
    rec = b">contig%06d some description\n" + (b"ACGTTGCAAGGCTTAACCGGTTAACCGGTTAAGGCCTTAAGGCCAATTGGCCAATTGGCCAATTGG\n" * 6)
    return b"".join(rec % i for i in range(max(n // len(rec % 0), 1)))


def _sam(n):
    rec = b"r%06d\t0\tchr1\t1000\t60\t36M\t*\t0\t0\tACGTACGTACGTACGTACGTACGTACGTACGTACGT\tIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"
    return b"@A x\n" + b"".join(rec % i for i in range(max(n // len(rec % 0), 1)))


def _line(n):
    return b"".join(b"line %06d of some plain text, about fifty bytes\n" % i for i in range(max(n // 50, 1)))


MAKE = {"fastq": _fastq, "fasta": _fasta, "sam": _sam, "line": _line}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--sizes", default="4096,65536,262144,1048576,4194304")
    ap.add_argument("--loop-nodes", type=int, default=64, help="nodes of the Python loop (scaled to --nodes)")
    a = ap.parse_args()
    ctx = Context(0)
    out = {"metric": "batch build of K nodes, device-resident", "unit": "ms", "steps": a.steps, "warmup": 2,
           "nodes": a.nodes, "build": "hipcc -O3 --offload-arch=gfx950", "sizes": {}, "formats": {}}

    def timed(fn):
        for _ in range(2):
            fn()
        ws, ks = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            r = fn()
            ws.append((time.perf_counter() - t0) * 1e3)
            ks.append(r.timings.get("kernel_ms", 0.0) if hasattr(r, "timings") else r)
        return {"call_ms": round(float(np.median(ws)), 4), "device_ms": round(float(np.median(ks)), 4),
                "call_min": round(min(ws), 4), "call_max": round(max(ws), 4)}

    def one(fmt, size, K):
        body = MAKE[fmt](size)
        stride = (len(body) + 15) & ~15
        arena = np.zeros(stride * K, dtype=np.uint8)
        arena.reshape(K, stride)[:, :len(body)] = np.frombuffer(body, dtype=np.uint8)
        nodes = np.stack([np.arange(K, dtype=np.int64) * stride, np.full(K, len(body), dtype=np.int64)], axis=1)
        d = ctx.alloc(arena.nbytes + 64, node=True)
        d.upload(arena)
        dn = ctx.alloc(nodes.nbytes + 64)
        dn.upload(nodes)
        cap = K * (len(body) // 16 + 16)
        rows = ctx.alloc(16 * cap)
        kind, f = ("line", None) if fmt == "line" else ("record", fmt)

        def batch():
            r = ctx.build_batch_device(d.ptr, arena.nbytes, dn.ptr, K, rows.ptr, cap, kind, f)
            assert r.ok and r.count == K, (r.status, r.err, r.count)
            return r

        res = {"node_bytes": len(body)}
        os.environ["SHOCKIDX_BATCH_SMALL"] = str(1 << 40)
        res["batch"] = timed(batch)
        res["batch"]["stats"] = ctx.batch_stats()
        os.environ["SHOCKIDX_BATCH_SMALL"] = "0"
        res["singles"] = timed(batch)
        del os.environ["SHOCKIDX_BATCH_SMALL"]
        kl = min(a.loop_nodes, K)

        def loop():
            ms = 0.0
            for i in range(kl):
                r = ctx.build_device(d.ptr + i * stride, len(body), rows.ptr, cap, kind, f)
                assert r.ok
                ms += r.timings["kernel_ms"]
            return ms

        lp = timed(loop)
        res["loop"] = {k: round(v * K / kl, 4) for k, v in lp.items()}
        for b in (d, dn, rows):
            b.free()
        return res

    for size in [int(x) for x in a.sizes.split(",")]:
        K = a.nodes if size * a.nodes <= (1 << 30) else max((1 << 30) // size, 1)
        out["sizes"][str(size)] = dict(one("fastq", size, K), nodes=K)
    for fmt in ("fasta", "sam", "line"):
        out["formats"][fmt] = dict(one(fmt, 65536, a.nodes), nodes=a.nodes)
    out["few"] = {}
    for K in (1, 8, 64):
        for size in (4096, 16384, 65536, 262144):
            r = one("fastq", size, K)
            out["few"][f"{K}x{size}"] = {"batch_ms": r["batch"]["call_ms"], "singles_ms": r["singles"]["call_ms"]}
    out["thousand_8k"] = dict(one("fastq", 8192, 1000), nodes=1000)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
