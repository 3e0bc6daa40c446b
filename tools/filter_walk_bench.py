"""The download filters over a node file: the whole path against the slab walk, and the oracle as the
reference's stand-in, over one synthetic FASTQ file read from the page cache:
  whole   shockidx_filter_fd on an uncapped context (asserted from its stats to take the whole path:
          the section, its output and the workspace resident at once)
  walk    shockidx_filter_fd on a context capped at --cap bytes (asserted to take the walk and to hold
          no more than the cap)
  oracle  oracle/filter_oracle.c on one CPU thread over the same bytes (mapped), output in memory
for fq2fa and anonymize, with out_fd at /dev/null and at a file on the same tmpfs.  The arms are whole
calls, plumbing included: file to device, filter, output to the host, write(2).  Times are medians of
the call's wall time over --steps calls after one warm-up call; the walk's kernel / D2H / write split
comes from shockidx_filter_last_stats.  The outputs written to the tmpfs file are hashed and compared
across the three arms, and the walk over the file's first 256 MiB is compared byte for byte with the
oracle's.  Prints one JSON line and writes it to --out.  Dev tool; tests/test_gpu_filter_slabs.py
carries the parity cases."""
import argparse
import hashlib
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shock_amd import Context, _lib as L  # noqa: E402
import gen  # noqa: E402
import oracle  # noqa: E402


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def oracle_sha(data, name):
    """oracle_filter_fastq over data (a uint8 array), its output hashed where it lies (oracle.filter_fastq returns
    the stream as one bytes object, which ctypes cannot make above 2 GiB): (records, bytes, sha256, seconds)"""
    import ctypes
    out_p = ctypes.POINTER(ctypes.c_uint8)()
    outlen, count = ctypes.c_size_t(0), ctypes.c_uint64(0)
    err = ctypes.create_string_buffer(256)
    t0 = time.perf_counter()
    rc = oracle.lib().oracle_filter_fastq(data.ctypes.data, data.size, oracle.FILTERS[name], ctypes.byref(out_p),
                                          ctypes.byref(outlen), ctypes.byref(count), err, 256)
    dt = time.perf_counter() - t0
    assert rc == 0, (rc, err.value)
    h = hashlib.sha256(np.ctypeslib.as_array(out_p, shape=(outlen.value,))).hexdigest() if outlen.value else ""
    oracle.lib().oracle_free(ctypes.cast(out_p, ctypes.c_void_p))
    return int(count.value), int(outlen.value), h, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=1 << 30)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter", "bench_filter_walk.json"))
    a = ap.parse_args()
    size = int(a.gib * (1 << 30))
    block = gen.fastq(random.Random(5), 4000, plus_id=0.2)
    res = {"metric": "download filters over a node file: whole path vs slab walk vs oracle (one CPU thread)",
           "unit": "GiB/s of input, whole calls (file to device, filter, output to host, write)", "steps": a.steps,
           "warmup": 1, "file_bytes": 0, "cap_bytes": a.cap, "build": "hipcc -O3 --offload-arch=gfx950", "filters": {}}
    with tempfile.TemporaryDirectory(dir=a.tmp) as td:
        path, outp = os.path.join(td, "body.fq"), os.path.join(td, "out.bin")
        with open(path, "wb") as f:
            for _ in range(size // len(block) + 1):
                f.write(block)
        n = os.path.getsize(path)
        res["file_bytes"] = n
        fd = os.open(path, os.O_RDONLY)
        data = np.memmap(path, dtype=np.uint8, mode="r")
        head = min(n, 256 << 20)

        def timed(ctx, name, target, m=n):
            ws, r = [], None
            for i in range(a.steps + 1):
                w = os.open(target, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
                t0 = time.perf_counter()
                r = ctx.filter_fd(name, fd, 0, m, w)
                dt = time.perf_counter() - t0
                os.close(w)
                assert r.status == L.OK, (r.status, r.err)
                if i:
                    ws.append(dt)
            return r, {"gib_s": round(m / float(np.median(ws)) / (1 << 30), 3),
                       "gib_s_min": round(m / max(ws) / (1 << 30), 3), "gib_s_max": round(m / min(ws) / (1 << 30), 3)}

        for name in ("fq2fa", "anonymize"):
            fr = {}
            o_n, o_bytes, o_sha, dt = oracle_sha(np.asarray(data), name)
            fr["oracle"] = {"gib_s": round(n / dt / (1 << 30), 3), "records": o_n, "out_bytes": o_bytes, "sha256": o_sha}
            for arm, cap in (("whole", 0), ("walk", a.cap)):
                ctx = Context(0)
                ctx.set_dev_cap(cap)
                fr[arm] = {}
                for tname, target in (("devnull", "/dev/null"), ("tmpfs", outp)):
                    r, t = timed(ctx, name, target)
                    st = ctx.filter_stats()
                    assert st["path"] == (1 if arm == "whole" else 2), st
                    assert (r.count, r.size) == (fr["oracle"]["records"], fr["oracle"]["out_bytes"])
                    t.update(peak_bytes=st["peak_bytes"], slabs=st["slabs"], restarts=st["restarts"],
                             slab_bytes=st["slab_bytes"], halo_bytes=st["halo_bytes"], kernel_ms=round(st["kernel_us"] / 1e3, 1),
                             d2h_ms=round(st["d2h_us"] / 1e3, 1), write_ms=round(st["write_us"] / 1e3, 1),
                             total_ms=round(r.total_ms, 1))
                    if tname == "tmpfs":
                        t["sha256"] = sha(outp)
                    fr[arm][tname] = t
                if arm == "walk":
                    assert fr[arm]["tmpfs"]["peak_bytes"] <= a.cap
                    # the first 256 MiB (it ends inside a record) against the oracle, byte for byte
                    w = os.open(outp, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
                    r = ctx.filter_fd(name, fd, 0, head, w)
                    os.close(w)
                    want, k, err = oracle.filter_fastq(np.asarray(data[:head]), name)
                    with open(outp, "rb") as f:
                        got = f.read()
                    fr["head_256mib_equal"] = bool(got == want and r.count == k and
                                                   (r.status, r.err) == ((L.EFORMAT, err) if err else (L.OK, None)))
                ctx.close()
            fr["hashes_equal"] = fr["whole"]["tmpfs"]["sha256"] == fr["walk"]["tmpfs"]["sha256"] == fr["oracle"]["sha256"]
            fr["walk_over_whole_devnull"] = round(fr["walk"]["devnull"]["gib_s"] / fr["whole"]["devnull"]["gib_s"], 3)
            res["filters"][name] = fr
        del data
        os.close(fd)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
