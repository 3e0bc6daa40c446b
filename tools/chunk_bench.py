"""chunkrecord over page-cached node files: the whole-node build against the slab walk.

Two nodes of --gib GiB, a FASTQ and a FASTA one, are written to a temporary directory (--tmp: e.g. a
tmpfs) by repeating a seeded block and read once, so they sit in the page cache.
Per node three arms, each in a child process of its own (a process loads one library):
  whole   shockidx_chunkrecord_fd without a device cap: the whole-node build
  walk    the same entry under a --cap-mib device cap: the slab walk (result.path 6)
  parent  the parent commit's library (shock_amd/variants/libshockidx_parent.so: libshockidx.so as
          `make -C shock_amd/csrc` builds it in a checkout of the parent commit, copied there and loaded
          with SHOCKIDX_VARIANT=parent) through its shockidx_chunkrecord_fd, on the same files
Per arm: 3 warm-up and --steps timed builds; the median wall ms, GiB/s, the spread (max - min) of the
timed builds and the device bytes the context held after them; the table is hashed and must be equal
across arms.  Prints one JSON line and writes it to --out.  Dev tool; the GPU tests carry the parity cases."""
import argparse
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def fastq_block(rng, k):
    """Records the record index accepts (bare '+' lines, so the speculative build has its node positions;
    tests/test_oracle_chunk.py's generator names some '+' lines, which ends the record table early)."""
    out = []
    for i in range(k):
        L = rng.randint(50, 300)
        seq = bytes(rng.choice(b"ACGTN") for _ in range(64)) * (L // 64 + 1)
        q = bytes(rng.randint(35, 74) for _ in range(64)) * (L // 64 + 1)
        out.append(b"@r%d x\n%s\n+\n%s\n" % (i, seq[:L], q[:L]))
    return b"".join(out)


def make_file(path, fmt, size):
    from test_oracle_chunk import fasta_records
    rng = random.Random(7)
    block = fastq_block(rng, 30000) if fmt == "fastq" else fasta_records(rng, 5000)
    reps = max(1, size // len(block))
    with open(path, "wb") as f:
        for _ in range(reps):
            f.write(block)
    with open(path, "rb") as f:  # (read once: the pages are in the cache)
        while f.read(64 << 20):
            pass
    return reps * len(block)


def arm_main(a):
    from shock_amd import Context
    ctx = Context(0)
    if a.cap_mib and a.arm == "walk":
        ctx.set_dev_cap(a.cap_mib << 20)
    size = os.path.getsize(a.file)
    fd = os.open(a.file, os.O_RDONLY)
    walls, r = [], None
    for i in range(3 + a.steps):
        t0 = time.perf_counter()
        r = ctx.chunkrecord_fd(fd, size)
        dt = (time.perf_counter() - t0) * 1e3
        if r.status != 0:
            raise RuntimeError(f"{a.arm}: status {r.status} {r.err}")
        if i >= 3:
            walls.append(dt)
    os.close(fd)
    med = float(np.median(walls))
    out = {"arm": a.arm, "bytes": size, "path": r.path, "rows": r.count, "rounds": r.reruns,
           "wall_ms": round(med, 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
           "spread_ms": round(max(walls) - min(walls), 3), "gib_s": round(size / (med * 1e-3) / (1 << 30), 2),
           "device_ms": round(r.timings["kernel_ms"], 3), "device_bytes": ctx.workspace_bytes(),
           "hash": hashlib.blake2b(np.ascontiguousarray(r.rows, dtype="<u8").tobytes(), digest_size=16).hexdigest()}
    print("ARM " + json.dumps(out))
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cap-mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk", "bench_chunk_slabs.json"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--arm", default=None, help="(internal) run one arm over --file")
    ap.add_argument("--file", default=None)
    a = ap.parse_args()
    if a.arm:
        return arm_main(a)
    out = {"metric": "chunkrecord over a page-cached node file: whole-node build, slab walk, parent's whole-node build",
           "unit": "ms", "steps": a.steps, "warmup": 3, "cap_bytes": a.cap_mib << 20,
           "build": "hipcc -O3 --offload-arch=gfx950"}
    ok = True
    with tempfile.TemporaryDirectory(dir=a.tmp) as td:
        for fmt in ("fastq", "fasta"):
            path = os.path.join(td, "node." + fmt)
            size = make_file(path, fmt, int(a.gib * (1 << 30)))
            arms = {}
            for arm in ("parent", "whole", "walk"):
                env = dict(os.environ)
                env.pop("SHOCKIDX_DEV_CAP", None)
                if arm == "parent":
                    env["SHOCKIDX_VARIANT"] = "parent"
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--file", path, "--steps",
                                    str(a.steps), "--cap-mib", str(a.cap_mib)], env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.STDOUT, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("ARM ")]
                if p.returncode != 0 or not line:
                    print(p.stdout, file=sys.stderr)
                    raise RuntimeError(f"arm {arm} over {fmt} failed")
                arms[arm] = json.loads(line[0][4:])
            par = arms["parent"]
            for arm in ("whole", "walk"):
                e = arms[arm]
                e["vs_parent"] = round(e["wall_ms"] / par["wall_ms"], 4)
                e["minus_parent_ms"] = round(e["wall_ms"] - par["wall_ms"], 3)
                e["within_3_spreads_of_parent"] = bool(e["wall_ms"] - par["wall_ms"] <= 3 * par["spread_ms"])
            same = len({e["hash"] for e in arms.values()}) == 1 and len({e["rows"] for e in arms.values()}) == 1
            ok = ok and same and arms["walk"]["path"] == 6 and arms["whole"]["path"] != 6
            out[fmt] = {"bytes": size, "tables_equal": bool(same), **arms}
    out["tables_ok"] = bool(ok)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
