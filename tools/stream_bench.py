"""The sectioned stream on the device: a filtered download of a 1 % subset of a FASTQ node
(subset_node -> idx_range -> stream_filter_device, fq2fa and anonymize) next to two references
measured in the same process:
  gather      shockidx_subset_gather of the same runs -- the unfiltered lower bound
  per_section the loop the library offered before: one run copied out (a one-run gather, the
              single-section entry point wants a 16-byte aligned section) and shockidx_filter_device on
              it, over the first --loop-runs runs, scaled to the run count
and the A/B behind the small-section limit (SHOCKIDX_STREAM_SMALL): the segmented path against the
single-section path over the same list of record-aligned sections of about 4 KiB, 64 KiB and 1 MiB.
The body is a SynthFile FASTQ node of --mib MiB in HBM.  Times are medians over --steps calls after
3 warm-up calls; device_ms is the call's HIP-event time, call_ms its wall time (the host's waits
included).  Prints one JSON line.  Dev tool; the GPU tests carry the parity cases.
--fmt fasta | sam: the same two tables for anonymize over FASTA / SAM sections (other_format)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shock_amd import Context  # noqa: E402
from shock_amd.synth import SynthFile  # noqa: E402


SAM_HEAD = b"@A x\n"  # sam.go:17: a section detects as SAM by its first line


def _sam_line(i):
    return b"r%d\t0\tchr1\t%d\t60\t36M\t*\t0\t0\tACGTACGTACGTACGTACGTACGTACGTACGTACGT\tIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" % (
        i, i % 100000 + 1)


def _sam_node(nblocks, lines):
    """nblocks sections of SAM_HEAD + `lines` alignment lines, back to back -> (bytes, [[pos, len]])."""
    blk = [SAM_HEAD + b"".join(_sam_line(17 * b + j) for j in range(lines)) for b in range(min(nblocks, 64))]
    parts = [blk[i % len(blk)] for i in range(nblocks)]
    pos = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    return b"".join(parts), np.stack([pos[:-1], np.diff(pos)], axis=1).astype(np.int64)


def other_format(a):
    """--fmt fasta | sam: anonymize over small FASTA / SAM sections.  The two tables of the FASTQ run:
    the subset-sized list (the runs of a --frac id subset of a SynthFile FASTA node; for SAM, every
    1 / --frac-th block of a node of header + 3 alignment lines, since only a section that starts with a
    header line detects as SAM) against the plain gather, against the per-section loop and against the
    same call with every section on the single-section path (SHOCKIDX_STREAM_SMALL=0: what the call did
    before the segmented FASTA / SAM path), both over the first --loop-runs runs and scaled; and the
    segmented path against the single-section path at 1 and --ab-sections sections of about 2.8 KiB,
    64 KiB and 1 MiB.  Medians over --steps calls after 3 warm-up calls, with min and max."""
    n = a.mib << 20
    ctx = Context(0)
    out = {"metric": f"sectioned download filter (anonymize, {a.fmt} sections), device-resident", "unit": "ms",
           "steps": a.steps, "warmup": 3, "build": "hipcc -O3 --offload-arch=gfx950"}

    def timed(fn, steps=a.steps, warm=3):
        for _ in range(warm):
            r = fn()
        ks, ws = [], []
        for _ in range(steps):
            t = time.perf_counter()
            r = fn()
            ws.append((time.perf_counter() - t) * 1e3)
            ks.append(r.kernel_ms)
        return r, {"device_ms": round(float(np.median(ks)), 4), "call_ms": round(float(np.median(ws)), 4),
                   "call_ms_min": round(min(ws), 4), "call_ms_max": round(max(ws), 4)}

    if a.fmt == "fasta":
        sf = SynthFile(ctx, "fasta", n)
        data = sf.window(0, n)
        R = sf.expected_count()
        rows = ctx.alloc(16 * (R + 1024))
        r = ctx.build_buffer(data, n, rows, kind="record", fmt="fasta")
        assert r.ok and r.count == R
        tab = rows.rows(R).astype(np.int64)
        ids = np.sort(np.random.default_rng(5).choice(R, size=max(1, int(R * a.frac)), replace=False))
        brk = np.flatnonzero(np.diff(ids) != 1) + 1  # the maximal runs of consecutive records
        first, last = ids[np.concatenate([[0], brk])], ids[np.concatenate([brk - 1, [len(ids) - 1]])]
        runs = np.stack([tab[first, 0], tab[last, 0] + tab[last, 1] - tab[first, 0]], axis=1).astype(np.int64)

        def sections(size, count):
            per = max(1, round(size / (n / R)))
            ns = min(count, R // per)
            return np.array([[tab[i * per, 0], tab[(i + 1) * per - 1, 0] + tab[(i + 1) * per - 1, 1] - tab[i * per, 0]]
                             for i in range(ns)], dtype=np.int64)
        out.update(bytes=n, records=R, ids=len(ids))
    else:
        host, blocks = _sam_node(max(64, min(n // 350, 2_000_000)), 3)
        n = len(host)
        data = ctx.alloc(n + 64)
        data.upload(host)
        runs = blocks[::max(1, int(round(1 / a.frac)))].copy()
        ab_nodes = {}

        def sections(size, count):
            lines = max(1, size // 114)
            h, s = _sam_node(count, lines)
            d = ctx.alloc(len(h) + 64)
            d.upload(h)
            ab_nodes[size] = (d, len(h))
            return s
        out.update(bytes=n, blocks=len(blocks))
    nruns = len(runs)
    d_recs = ctx.alloc(16 * nruns + 64)
    d_recs.upload(runs.tobytes())
    total = int(runs[:, 1].sum())
    out.update(runs=nruns, subset_bytes=total, mean_run_bytes=round(total / nruns, 1))
    cap = 2 * total + 4096
    d_out = ctx.alloc(cap)
    g, gt = timed(lambda: ctx.subset_gather(data.ptr, n, d_recs.ptr, nruns, d_out.ptr, cap))
    assert g.ok and g.size == total
    out["gather"] = gt
    os.environ.pop("SHOCKIDX_STREAM_SMALL", None)
    s, st = timed(lambda: ctx.stream_filter_device("anonymize", data.ptr, n, d_recs.ptr, nruns, d_out.ptr, cap))
    assert s.ok, (s.status, s.err)
    e = dict(st, items=s.count, bytes_out=s.size, stats=ctx.stream_stats(),
             vs_gather_call=round(st["call_ms"] / gt["call_ms"], 2))
    m = min(a.loop_runs, nruns)
    d_one = ctx.alloc(int(runs[:, 1].max()) + 64)

    def loop():
        cnt = 0
        for i in range(m):
            ln = int(runs[i, 1])
            ctx.subset_gather(data.ptr, n, d_recs.ptr + 16 * i, 1, d_one.ptr, ln)
            cnt += ctx.filter_device("anonymize", d_one.ptr, ln, d_out.ptr, cap).count
        return cnt
    loop()
    t = time.perf_counter()
    cnt = loop()
    lw = (time.perf_counter() - t) * 1e3
    e["per_section"] = {"runs_timed": m, "items": cnt, "call_ms_timed": round(lw, 2),
                        "call_ms_scaled": round(lw * nruns / m, 1), "speedup_call": round(lw * nruns / m / st["call_ms"], 1)}
    os.environ["SHOCKIDX_STREAM_SMALL"] = "0"  # every section on the single-section path: the call as it was
    p, pt = timed(lambda: ctx.stream_filter_device("anonymize", data.ptr, n, d_recs.ptr, m, d_out.ptr, cap), steps=3, warm=1)
    assert p.ok and ctx.stream_stats()["singles"] == m
    os.environ.pop("SHOCKIDX_STREAM_SMALL", None)
    q, qt = timed(lambda: ctx.stream_filter_device("anonymize", data.ptr, n, d_recs.ptr, m, d_out.ptr, cap))
    assert (q.count, q.size) == (p.count, p.size)
    e["single_path_call"] = {"runs_timed": m, "call_ms_timed": pt["call_ms"], "call_ms_scaled": round(pt["call_ms"] * nruns / m, 1),
                             "segmented_call_ms_same_runs": qt["call_ms"],
                             "speedup_call": round(pt["call_ms"] / qt["call_ms"], 1)}
    out["anonymize"] = e

    ab = {}
    for size in (2867, 64 << 10, 1 << 20):
        secs = sections(size, a.ab_sections)
        ns = len(secs)
        d_secs = ctx.alloc(16 * ns + 64)
        d_secs.upload(secs.tobytes())
        src, src_n = (data, n) if a.fmt == "fasta" else ab_nodes[size]
        need = 2 * int(secs[:, 1].sum()) + 4096
        if need > cap:
            d_out.free()
            cap = need
            d_out = ctx.alloc(cap)
        for count in sorted({1, ns}):
            row = {"section_bytes": int(round(float(secs[:count, 1].mean())))}
            res = {}
            for path, limit in (("segmented", str(16 << 20)), ("single", "0")):
                os.environ["SHOCKIDX_STREAM_SMALL"] = limit
                s, t = timed(lambda: ctx.stream_filter_device("anonymize", src.ptr, src_n, d_secs.ptr, count, d_out.ptr, cap))
                assert s.ok, (size, count, path, s.status, s.err)
                stt = ctx.stream_stats()
                assert (stt["batches"], stt["singles"]) == ((1, 0) if path == "segmented" else (0, count)), stt
                res[path] = (s.count, s.size)
                row.update({f"{path}_{k}": v for k, v in t.items()})
            assert res["segmented"] == res["single"], res
            os.environ.pop("SHOCKIDX_STREAM_SMALL", None)
            row["segmented_wins"] = row["segmented_call_ms"] < row["single_call_ms"]
            ab[f"{size}B_x{count}"] = row
        d_secs.free()
    out["small_limit_ab"] = ab
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fmt", choices=("fastq", "fasta", "sam"), default="fastq")
    ap.add_argument("--mib", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frac", type=float, default=0.01)
    ap.add_argument("--loop-runs", type=int, default=2000)
    ap.add_argument("--ab-sections", type=int, default=64)
    a = ap.parse_args()
    if a.fmt != "fastq":
        return other_format(a)
    n = a.mib << 20
    ctx = Context(0)
    sf = SynthFile(ctx, "fastq", n)
    data = sf.window(0, n)
    R = sf.expected_count()
    rows = ctx.alloc(16 * (R + 1024))
    r = ctx.build_buffer(data, n, rows, kind="record", fmt="fastq")
    assert r.ok and r.count == R
    out = {"metric": "sectioned download filter, device-resident", "bytes": n, "records": R, "unit": "ms",
           "steps": a.steps, "warmup": 3, "build": "hipcc -O3 --offload-arch=gfx950"}

    def timed(fn, steps=a.steps, warm=3):
        for _ in range(warm):
            r = fn()
        ks, ws = [], []
        for _ in range(steps):
            t = time.perf_counter()
            r = fn()
            ws.append((time.perf_counter() - t) * 1e3)
            ks.append(r.kernel_ms)
        return r, float(np.median(ks)), float(np.median(ws))

    # the subset node: a seeded id list, its rows and runs, and Range over its rows -- all on the device
    ids = np.sort(np.random.default_rng(5).choice(R, size=max(1, int(R * a.frac)), replace=False) + 1)
    text = ("\n".join(map(str, ids.tolist())) + "\n").encode()
    k = len(ids)
    d_ids, d_srows, d_runs, d_recs = ctx.alloc(len(text) + 64), ctx.alloc(16 * k + 64), ctx.alloc(16 * k + 64), \
        ctx.alloc(16 * k + 64)
    d_ids.upload(text)
    d_gath = ctx.alloc(n // 8 + 64)
    sn = ctx.subset_node(d_ids.ptr, len(text), rows.ptr, R, R, d_srows.ptr, k, d_runs.ptr, k, data.ptr, n, d_gath.ptr,
                         n // 8)
    assert sn.ok and sn.count == k
    nruns, err = ctx.idx_range(d_srows.ptr, k, f"1-{k}", k, d_recs.ptr, k)
    assert err is None and nruns == sn.runs
    out.update(ids=k, runs=nruns, subset_bytes=sn.size, mean_run_bytes=round(sn.size / nruns, 1))
    cap = 2 * sn.size + 64
    d_out = ctx.alloc(cap)
    g, ms, wall = timed(lambda: ctx.subset_gather(data.ptr, n, d_recs.ptr, nruns, d_out.ptr, cap))
    assert g.ok and g.size == sn.size
    out["gather"] = {"device_ms": round(ms, 4), "call_ms": round(wall, 4)}
    runs = d_recs.rows(nruns).view(np.int64)
    d_one = ctx.alloc(int(runs[:, 1].max()) + 64)
    for name in ("fq2fa", "anonymize"):
        s, ms, wall = timed(lambda: ctx.stream_filter_device(name, data.ptr, n, d_recs.ptr, nruns, d_out.ptr, cap))
        assert s.ok and s.count == k, (s.status, s.err, s.count)
        e = {"records": s.count, "bytes_out": s.size, "device_ms": round(ms, 4), "call_ms": round(wall, 4),
             "vs_gather_call": round(wall / out["gather"]["call_ms"], 2)}
        m = min(a.loop_runs, nruns)

        def loop():
            cnt = 0
            for i in range(m):
                ln = int(runs[i, 1])
                ctx.subset_gather(data.ptr, n, d_recs.ptr + 16 * i, 1, d_one.ptr, ln)
                cnt += ctx.filter_device(name, d_one.ptr, ln, d_out.ptr, cap).count
            return cnt
        loop()
        t = time.perf_counter()
        cnt = loop()
        lw = (time.perf_counter() - t) * 1e3
        e["per_section"] = {"runs_timed": m, "records": cnt, "call_ms_timed": round(lw, 2),
                            "call_ms_scaled": round(lw * nruns / m, 1), "speedup_call": round(lw * nruns / m / wall, 1)}
        out[name] = e

    # the small-section limit: both paths over the same sections (record-aligned, about `size` bytes)
    tab = rows.rows(R)
    ab = {}
    for size in (4 << 10, 64 << 10, 1 << 20):
        per = max(1, int(size / (n / R)))
        ns = min(a.ab_sections, R // per)
        secs = np.array([[tab[i * per, 0], tab[(i + 1) * per - 1, 0] + tab[(i + 1) * per - 1, 1] - tab[i * per, 0]]
                         for i in range(ns)], dtype=np.int64)
        d_secs = ctx.alloc(16 * ns + 64)
        d_secs.upload(secs.tobytes())
        if 2 * int(secs[:, 1].sum()) + 64 > cap:
            d_out.free()
            cap = 2 * int(secs[:, 1].sum()) + 64
            d_out = ctx.alloc(cap)
        for count in sorted({1, ns}):
            for name in ("fq2fa", "anonymize"):
                row = {"section_bytes": int(secs[0, 1])}
                for path, limit in (("segmented", str(16 << 20)), ("single", "0")):
                    os.environ["SHOCKIDX_STREAM_SMALL"] = limit
                    s, ms, wall = timed(lambda: ctx.stream_filter_device(name, data.ptr, n, d_secs.ptr, count, d_out.ptr,
                                                                         cap), steps=max(3, a.steps // 2), warm=2)
                    assert s.ok and s.count == per * count, (size, count, name, path, s.status, s.err, s.count)
                    row[path + "_call_ms"] = round(wall, 4)
                    row[path + "_device_ms"] = round(ms, 4)
                os.environ.pop("SHOCKIDX_STREAM_SMALL", None)
                ab[f"{size >> 10}KiB_x{count}_{name}"] = row
        d_secs.free()
    out["small_limit_ab"] = ab
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
