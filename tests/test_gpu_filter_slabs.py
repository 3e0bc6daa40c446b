"""GPU: the download filters in slabs -- shockidx_filter_slab_device (one slab of a FASTQ section with
the reader's position and the filter's counter in a device carry), shockidx_filter_fd_walk (a section
of a file through two slots to a descriptor) and shockidx_filter_fd (the whole path or the walk,
inside the context's device cap).  Every stream, count, status and text is compared with the oracle
(oracle/filter_oracle.c) over the same bytes; the per-slab counts with the oracle's record index.

The node is resident in one buffer and slabs are windows of it.  A slab's d_data must be 16-byte
aligned, so every slab after the first starts its window at the carried position rounded down to 16
(front 0: no byte before the carried position is needed).  Two ways to cut: "window" -- the slab
reads and owns [base, cut) (n = end) -- and "owned" -- the slab reads to the section's end and owns
[base, cut) (n < end).  anonymize's first slab must hold the section's first min(32768, size) bytes
(detection reads them), so a section under 32 KiB can be cut under anonymize only by ownership; the
window cuts of small sections run under anonymize behind a 32 KiB prefix of valid records."""
import os
import random
import threading

import numpy as np
import pytest

import gen
from test_gpu_filter import KATS

pytestmark = pytest.mark.gpu
NAMES = ("fq2fa", "anonymize")
DETECT = 32768
KIB, MIB = 1 << 10, 1 << 20


class Node:
    """a section resident in one device buffer, with an output buffer that holds any slab's output"""

    def __init__(self, ctx, data):
        self.ctx, self.data, self.size = ctx, data, len(data)
        self.buf = ctx.alloc(len(data) + 64)
        self.buf.upload(data)
        self.out = ctx.alloc(3 * len(data) + 256)

    def free(self):
        self.buf.free()
        self.out.free()


def walk(node, name, bounds, mode="window", halo=0):
    """The section slab by slab: every slab owns up to the next of `bounds` (section offsets, the
    section's size appended) past the carried position; a slab that could deliver nothing takes the
    bound after.  Returns (stream, count, status, err, log); log: one dict per slab."""
    ctx, sec = node.ctx, node.size
    bounds = sorted(set(b for b in bounds if 0 <= b < sec)) + [sec]
    carry = ctx.filter_carry()
    carry.fill(0xAB)  # (the first slab initialises it)
    pos, i, first, out, log = 0, 0, True, [], []
    for _ in range(4 * len(bounds) + 8):
        own_end = bounds[i]
        base = pos & ~15
        whi = sec if mode == "owned" else min(sec, own_end + halo)
        if first and name == "anonymize":
            whi = max(whi, min(DETECT, sec))
        last = whi == sec
        n = (whi if last and mode == "window" else own_end) - base
        r = ctx.filter_slab(name, node.buf, base, 0, n, whi - base, sec, carry, node.out, first=first)
        assert r.status in (0, 1), (r.status, r.err, base, n, whi)
        st = ctx.filter_carry_state(carry)
        out.append(node.out.download(r.size).tobytes() if r.size else b"")
        log.append(dict(base=base, n=n, whi=whi, last=last, count=r.count, size=r.size, pos=r.next_pos,
                        status=r.status, carried=st["count"], owned_all=base + n == whi))
        assert st["pos"] == r.next_pos and st["bytes"] == sum(len(o) for o in out)
        assert r.next_pos >= pos
        first = False
        if r.status == 1 or st["ended"]:
            assert st["ended"]
            return b"".join(out), st["count"], r.status, r.err, log
        pos = r.next_pos
        nxt = next((j for j, b in enumerate(bounds) if b > pos), len(bounds) - 1)
        i = min(max(i + 1, nxt), len(bounds) - 1)
    raise AssertionError("the walk did not end")


def check_walk(node, oracle_lib, name, bounds, mode="window", halo=0, rows=None):
    if name == "anonymize" and oracle_lib.detect(node.data)[0] in ("fasta", "sam"):
        return []  # (not a FASTQ section: anonymize does not walk it)
    got, count, status, err, log = walk(node, name, bounds, mode, halo)
    out, n, oerr = oracle_lib.filter_fastq(node.data, name)
    assert (status, err) == (1 if oerr else 0, oerr), (name, bounds, mode, status, err, oerr)
    assert count == n and got == out, (name, bounds, mode, count, n, len(got), len(out))
    if rows is not None:  # the count rule: a slab that is not the last has settled the rows that end in its window
        for s in log:
            if not s["last"] and s["owned_all"]:
                want = [r for r in rows if r[0] < s["whi"] and r[0] + r[1] <= s["whi"]]
                assert s["carried"] == len(want), (name, s, len(want))
                assert s["pos"] == (int(want[-1][0] + want[-1][1]) if want else 0), (name, s)
    return log


def _rows(oracle_lib, data):
    rows, err = oracle_lib.record_index(data, "fastq")
    return [(int(a), int(b)) for a, b in rows], err


# ---- every cut ---------------------------------------------------------------------------------
THREE = b"@r1 x\nACGT\n+\nIIII\n" + b"@r2\r\nAC\r\n+r2\r\nII\r\n" + b"@r3\nACG\n+r3\nIII\n"


def _prefix():
    """valid records, a little over 32 KiB: anonymize's first slab may end anywhere behind it"""
    return gen.fq_fill(DETECT + 100)


def test_every_cut_fq2fa(gpu_ctx, oracle_lib):
    """Three records (one with a '+id' line, one CRLF) as two slabs cut at every byte offset, n = end
    on the first: the stream, the count and the status of the whole call, and after the first slab
    the rows that start before the cut and end at or before it."""
    rows, err = _rows(oracle_lib, THREE)
    assert err is None and len(rows) == 3 and 50 <= len(THREE) <= 70
    node = Node(gpu_ctx, THREE)
    for cut in range(len(THREE)):
        log = check_walk(node, oracle_lib, "fq2fa", [cut], rows=rows)
        if cut:
            assert log[0]["whi"] == cut and not log[0]["last"]
    node.free()


def test_every_cut_anonymize(gpu_ctx, oracle_lib):
    """The same under anonymize.  The section alone is shorter than 32 KiB, so its first slab must hold
    all of it: a first slab cut inside it is EINVAL (carry untouched), and the cuts run by ownership;
    behind a 32 KiB prefix the first slab's window is cut at every byte offset of the three records."""
    from shock_amd import _lib as L
    node = Node(gpu_ctx, THREE)
    carry = gpu_ctx.filter_carry()
    carry.fill(0x5A)
    before = carry.download().tobytes()
    r = gpu_ctx.filter_slab("anonymize", node.buf, 0, 0, 20, 20, len(THREE), carry, node.out, first=True)
    assert r.status == L.EINVAL and b"32 KiB" in r.err and carry.download().tobytes() == before
    rows, _ = _rows(oracle_lib, THREE)
    for cut in range(0, len(THREE), 3):
        log = check_walk(node, oracle_lib, "anonymize", [cut], mode="owned")
        # owned, not readable: the first slab delivers the records that start before the cut
        assert log[0]["count"] == sum(1 for a, _ in rows if a < cut)
    node.free()
    pre = _prefix()
    data = pre + THREE
    rows, err = _rows(oracle_lib, data)
    assert err is None
    node = Node(gpu_ctx, data)
    for cut in range(len(pre), len(data)):
        log = check_walk(node, oracle_lib, "anonymize", [cut], rows=rows)
        assert log[0]["whi"] == cut and not log[0]["last"]
    node.free()


@pytest.mark.parametrize("name", NAMES)
def test_owned_versus_readable(gpu_ctx, oracle_lib, name):
    """n < end: a record that starts in [base + n, base + end) is left to the next slab even when it
    is settled; one that starts before base + n and closes inside the halo is delivered."""
    pre = _prefix() if name == "anonymize" else b""
    data = pre + THREE + THREE
    rows, _ = _rows(oracle_lib, data)
    k = len(rows) - 6  # the first of the six trailing records
    e0, e1, e2 = (rows[k + j][0] + rows[k + j][1] for j in range(3))
    node = Node(gpu_ctx, data)
    carry = gpu_ctx.filter_carry()
    out, _, _ = oracle_lib.filter_fastq(data, name)
    # owns up to record k + 1's first byte exclusive; reads through record k + 2
    r = gpu_ctx.filter_slab(name, node.buf, 0, 0, e0, e2, len(data), carry, node.out, first=True)
    assert r.status == 0 and r.count == k + 1 and r.next_pos == e0
    # one byte more is owned: record k + 1 starts before base + n and closes inside the halo
    r = gpu_ctx.filter_slab(name, node.buf, 0, 0, e0 + 1, e1 + 3, len(data), carry, node.out, first=True)
    assert r.status == 0 and r.count == k + 2 and r.next_pos == e1
    got = node.out.download(r.size).tobytes()
    # the next slab starts at the carried position (front 0) and ends the stream
    base = e1 & ~15
    r = gpu_ctx.filter_slab(name, node.buf, base, 0, len(data) - base, len(data) - base, len(data), carry, node.out)
    assert r.status == 0 and r.next_pos == len(data) and gpu_ctx.filter_carry_state(carry)["ended"]
    assert got + node.out.download(r.size).tobytes() == out
    node.free()


# ---- random ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
def test_random_slabs(gpu_ctx, oracle_lib, seed):
    """test_filter_random_gpu's generator (its 16 seeds, corruptions included) cut into slabs of
    16 KiB + 1, of 4 KiB and of one random size each: streams and statuses equal; on the valid seeds
    the count rule holds for every slab that is not the last."""
    rng = random.Random(100 + seed)
    data = gen.fastq(rng, rng.randint(1, 3000), crlf=0.3 if seed % 3 == 0 else 0.0, plus_id=0.3,
                     long_every=97 if seed % 4 == 3 else 0, final_nl=seed % 4 != 1,
                     uni=0.1 if seed % 5 == 2 else 0.0)
    if seed % 2:
        data = gen.fastq_corrupt(rng, data, rng.choice(gen.FASTQ_CORRUPTIONS))
    rows, err = _rows(oracle_lib, data)
    valid = seed % 2 == 0 and err is None
    node = Node(gpu_ctx, data)
    rnd = []
    while sum(rnd) < len(data):
        rnd.append(rng.randint(1, 40000))
    cuts = {"16k+1": range(16 * KIB + 1, len(data), 16 * KIB + 1), "4k": range(4 * KIB, len(data), 4 * KIB),
            "random": list(np.cumsum(rnd))}
    for name in NAMES:
        for label, b in cuts.items():
            check_walk(node, oracle_lib, name, [int(x) for x in b], rows=rows if valid else None)
    node.free()


# ---- counter digits ----------------------------------------------------------------------------
def test_counter_digits(gpu_ctx, oracle_lib):
    """1001 records of about 20 bytes, slab ends between records 9/10, 99/100 and 999/1000: the
    counter's digit count changes on either side of a slab end (the section is under 32 KiB, so under
    anonymize the slabs are cut by ownership; fq2fa's windows are cut)."""
    recs = [b"@rd%d\nACGTAC\n+\nIIIIII\n" % (i % 7) for i in range(1001)]
    data = b"".join(recs)
    assert 19 <= len(data) / 1001 <= 22
    ends = np.cumsum([len(r) for r in recs])
    bounds = [int(ends[k - 1]) for k in (9, 99, 999)]  # record k + 1 (1-based) starts the next slab
    node = Node(gpu_ctx, data)
    log = check_walk(node, oracle_lib, "anonymize", bounds, mode="owned")
    assert [s["carried"] for s in log] == [9, 99, 999, 1001]
    # and with the slab end inside records 10, 100 and 1000 (they straddle it)
    check_walk(node, oracle_lib, "anonymize", [b + 7 for b in bounds], mode="owned")
    check_walk(node, oracle_lib, "fq2fa", bounds)
    node.free()
    # window cuts under anonymize: the same records behind the prefix (counters continue past 4 digits)
    pre = _prefix()
    npre = len(_rows(oracle_lib, pre)[0])
    node = Node(gpu_ctx, pre + data)
    first = 100 - npre if npre < 100 else 1000 - npre  # the record that gets counter 100 (or 1000)
    assert 0 < first < 1001
    cut = len(pre) + int(ends[first - 2])
    log = check_walk(node, oracle_lib, "anonymize", [cut, cut + 2000], rows=_rows(oracle_lib, pre + data)[0])
    assert log[0]["carried"] in (99, 999)
    node.free()


# ---- errors and ends ---------------------------------------------------------------------------
def _placements(node, oracle_lib, name, lo, hi):
    """cuts that put the bytes [lo, hi) -- the failing or final record -- in the first slab, across a
    slab end and in the last slab"""
    cuts = sorted({c for c in (lo - 1, lo, lo + 1, (lo + hi) // 2, hi - 1, hi, hi + 1) if 0 < c < node.size})
    for c in cuts:
        if name == "fq2fa" or c >= DETECT:
            check_walk(node, oracle_lib, name, [c])
        check_walk(node, oracle_lib, name, [c], mode="owned")


@pytest.mark.parametrize("name", NAMES)
def test_kats_in_slabs(gpu_ctx, oracle_lib, name):
    """test_gpu_filter.py's KATS alone, behind a 32 KiB prefix and before a valid tail (where the same
    bytes no longer end the file: the oracle says what they mean there)."""
    pre, tail = _prefix(), gen.fq_fill(300)
    for kat in KATS:
        for data, lo in ((kat, 0), (pre + kat, len(pre)), (kat + tail, 0), (pre + kat + tail, len(pre))):
            node = Node(gpu_ctx, data)
            if not data:
                check_walk(node, oracle_lib, name, [])
            else:
                _placements(node, oracle_lib, name, lo + max(0, len(kat) - 12), lo + len(kat))
            node.free()


@pytest.mark.parametrize("kind", gen.FASTQ_CORRUPTIONS)
def test_corruptions_in_slabs(gpu_ctx, oracle_lib, kind):
    rng = random.Random(sum(kind.encode()))
    good = gen.fastq(rng, 40, plus_id=0.3)
    data = gen.fastq_corrupt(rng, good, kind)
    for name in NAMES:
        sec = (_prefix() if name == "anonymize" else b"") + data
        _, k, err = oracle_lib.filter_fastq(sec, name)
        rows, _ = _rows(oracle_lib, sec)
        lo = rows[k - 1][0] + rows[k - 1][1] if 0 < k <= len(rows) else 0  # where the failing (or final) Read starts
        nl = sec.find(b"\n", lo)
        for _ in range(3):
            nl = sec.find(b"\n", nl + 1) if nl >= 0 else -1
        node = Node(gpu_ctx, sec)
        _placements(node, oracle_lib, name, lo, nl + 1 if nl >= 0 else len(sec))
        node.free()


@pytest.mark.parametrize("name", NAMES)
def test_blank_runs_and_open_ends(gpu_ctx, oracle_lib, name):
    """A blank-line run across a slab end, followed by a record (the blank-lines error) and by EOF (a
    clean end); a final quality line without '\\n' is dropped by the last slab only."""
    pre = _prefix() if name == "anonymize" else gen.fq_fill(200)
    rec = b"@q\nACGT\n+\nIIII\n"
    for tail in (b"\n\n\n\n" + rec, b"\n\n\n\n", b"\n\n\nXY", b"@z\nAC\n+\nII"):
        data = pre + rec + tail
        node = Node(gpu_ctx, data)
        at = len(pre) + len(rec)
        for cut in (at, at + 1, at + 2, at + 3, at + 4, len(data) - 1):
            log = check_walk(node, oracle_lib, name, [cut])
            if tail.startswith(b"\n") and at < cut <= at + 4 and cut < len(data):  # the run is not settled: left to the last slab
                assert log[0]["pos"] == at and log[0]["status"] == 0
        node.free()
    # the record whose quality line ends at EOF is delivered by a slab that is not the last ...
    data = pre + rec + b"@z\nAC\n+\nII"
    node = Node(gpu_ctx, data + b"\n" + rec)
    check_walk(node, oracle_lib, name, [len(data)])
    check_walk(node, oracle_lib, name, [len(data) + 1])
    node.free()


def test_slab_call_errors(gpu_ctx, oracle_lib):
    from shock_amd import _lib as L
    data = gen.fq_fill(3000)
    rows, _ = _rows(oracle_lib, data)
    node = Node(gpu_ctx, data)
    ctx = gpu_ctx
    carry = ctx.filter_carry()
    raw = lambda: carry.download().tobytes()  # noqa: E731
    cut = 1600
    # ESPACE: the bytes the slab needs, nothing written, the carry unchanged; the repeated call succeeds
    node.out.fill(0x77, 64)
    carry.fill(0x11)
    before = raw()
    r = ctx.filter_slab("fq2fa", node.buf, 0, 0, cut, cut, len(data), carry, node.out, first=True, out_cap=10)
    want = [x for x in rows if x[0] + x[1] <= cut]
    assert r.status == L.ESPACE and r.count == len(want) and r.size > 10
    assert raw() == before and bytes(node.out.download(64)) == b"\x77" * 64
    r2 = ctx.filter_slab("fq2fa", node.buf, 0, 0, cut, cut, len(data), carry, node.out, first=True, out_cap=r.size)
    assert r2.status == L.OK and r2.size == r.size and r2.count == len(want)
    # a carried position before the window: EINVAL, the carry unchanged
    before = raw()
    base = (r2.next_pos + 16) & ~15
    r = ctx.filter_slab("fq2fa", node.buf, base, 0, len(data) - base, len(data) - base, len(data), carry, node.out)
    assert r.status == L.EINVAL and b"outside" in r.err and raw() == before
    # ... and past the owned bytes
    r = ctx.filter_slab("fq2fa", node.buf, 0, 0, 16, cut, len(data), carry, node.out, first=False)
    assert r.status == L.EINVAL and raw() == before
    # the other filter's carry
    r = ctx.filter_slab("anonymize", node.buf, 0, 0, len(data), len(data), len(data), carry, node.out, first=False)
    assert r.status == L.EINVAL and raw() == before
    # is_last must say whether the window ends the section
    r = ctx.filter_slab("fq2fa", node.buf, 0, 0, cut, cut, len(data), carry, node.out, first=False, last=True)
    assert r.status == L.EINVAL and raw() == before
    # the walk ends; a call after that is EINVAL, the carry unchanged
    base = r2.next_pos & ~15
    r = ctx.filter_slab("fq2fa", node.buf, base, 0, len(data) - base, len(data) - base, len(data), carry, node.out)
    assert r.status == L.OK and r2.count + r.count == len(rows) and ctx.filter_carry_state(carry)["ended"]
    before = raw()
    r = ctx.filter_slab("fq2fa", node.buf, base, 0, len(data) - base, len(data) - base, len(data), carry, node.out)
    assert r.status == L.EINVAL and b"ended" in r.err and raw() == before
    node.free()
    # anonymize over FASTA bytes on the first slab: EINVAL with a text that says so; over b"": EFORMAT
    fa = Node(ctx, b">c1 x\nACGT\nAC\n>c2\nA\n")
    carry.fill(0x22)
    before = raw()
    r = ctx.filter_slab("anonymize", fa.buf, 0, 0, fa.size, fa.size, fa.size, carry, fa.out, first=True)
    assert r.status == L.EINVAL and b"FASTA" in r.err and raw() == before
    sam = Node(ctx, b"@A x\n" + b"r1\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\n" * 3)
    assert oracle_lib.detect(sam.data)[0] == "sam" and oracle_lib.detect(fa.data)[0] == "fasta"
    r = ctx.filter_slab("anonymize", sam.buf, 0, 0, sam.size, sam.size, sam.size, carry, sam.out, first=True)
    assert r.status == L.EINVAL and b"SAM" in r.err and raw() == before
    r = ctx.filter_slab("anonymize", fa.buf, 0, 0, 0, 0, 0, carry, fa.out, first=True)
    assert r.status == L.EFORMAT and r.err == b"Invalid file type for filter" and r.count == 0 and r.size == 0
    assert ctx.filter_carry_state(carry)["ended"]
    r = ctx.filter_slab("fq2fa", fa.buf, 0, 0, 0, 0, 0, carry, fa.out, first=True)  # fq2fa over an empty section
    assert r.status == L.OK and r.count == 0 and r.size == 0 and ctx.filter_carry_state(carry)["ended"]
    assert oracle_lib.filter_fastq(b"", "anonymize")[2] == b"Invalid file type for filter"
    fa.free()
    sam.free()


# ---- the walk over a file ----------------------------------------------------------------------
_FILE = {}


def _walk_file():
    """about 3 MiB of seeded records and the oracle's record index of it (made once)"""
    if not _FILE:
        rng = random.Random(2024)
        _FILE["data"] = gen.fastq(rng, 9500, crlf=0.1, plus_id=0.3)
        assert 2.5 * MIB < len(_FILE["data"]) < 4 * MIB
    return _FILE["data"]


def _to_file(ctx, name, path, off, n, tmp_path, **kw):
    outp = tmp_path / "out.bin"
    with open(path, "rb") as f, open(outp, "wb") as w:
        r = ctx.filter_fd_walk(name, f.fileno(), off, n, w.fileno(), **kw)
    return r, outp.read_bytes()


@pytest.mark.parametrize("name", NAMES)
def test_fd_walk_file_and_pipe(gpu_ctx, oracle_lib, tmp_path, name):
    from shock_amd import _lib as L
    data = _walk_file()
    p = tmp_path / "body.fq"
    p.write_bytes(data)
    out, n, err = oracle_lib.filter_fastq(data, name)
    assert err is None
    r, got = _to_file(gpu_ctx, name, p, 0, len(data), tmp_path, slab_bytes=64 * KIB, halo_bytes=4 * KIB)
    st = gpu_ctx.filter_stats()
    assert r.status == L.OK and (r.count, r.size) == (n, len(out)) and got == out
    assert st["path"] == 2 and st["slabs"] >= len(data) // (64 * KIB) and st["restarts"] == 0
    assert (st["slab_bytes"], st["halo_bytes"]) == (64 * KIB, 4 * KIB)
    # out_fd the write end of a pipe, drained by a thread
    rd, wr = os.pipe()
    chunks = []

    def drain():
        while True:
            b = os.read(rd, 1 << 16)
            if not b:
                return
            chunks.append(b)

    t = threading.Thread(target=drain)
    t.start()
    with open(p, "rb") as f:
        r = gpu_ctx.filter_fd_walk(name, f.fileno(), 0, len(data), wr, 64 * KIB, 4 * KIB)
    os.close(wr)
    t.join()
    os.close(rd)
    assert r.status == L.OK and b"".join(chunks) == out
    # a closed read end: SHOCKIDX_EIO with the errno text
    rd, wr = os.pipe()
    os.close(rd)
    with open(p, "rb") as f:
        r = gpu_ctx.filter_fd_walk(name, f.fileno(), 0, len(data), wr, 64 * KIB, 4 * KIB)
    os.close(wr)
    assert r.status == L.EIO and r.err.startswith(b"write: ")


@pytest.mark.parametrize("name", NAMES)
def test_fd_walk_sections(gpu_ctx, oracle_lib, tmp_path, name):
    """off = 12345 (mid-record) and a section that starts at a record, n ending mid-record: streams
    and errors are the oracle's over data[off:off + n]"""
    from shock_amd import _lib as L
    data = _walk_file()
    p = tmp_path / "body.fq"
    p.write_bytes(data)
    rows, _ = _rows(oracle_lib, data)
    at = next(a for a, _ in rows if a > 12345)
    for off, n in ((12345, 700001), (at, 700001), (at, rows[5000][0] + rows[5000][1] - at), (12345, 0), (len(data), 0)):
        sec = data[off:off + n]
        assert name == "fq2fa" or oracle_lib.detect(sec)[0] in ("fastq", None)
        out, k, err = oracle_lib.filter_fastq(sec, name)
        r, got = _to_file(gpu_ctx, name, p, off, n, tmp_path, slab_bytes=64 * KIB, halo_bytes=4 * KIB)
        assert (r.status, r.err) == ((L.EFORMAT, err) if err else (L.OK, None)), (off, n, r.status, r.err, err)
        assert r.count == k and got == out, (off, n)


def test_fd_walk_restart_and_nomem(gpu_ctx, oracle_lib, tmp_path):
    """A 50 KB record that starts near the end of a slab's owned bytes is not settled inside the 4 KiB
    halo: the next slab restarts at it in a fresh slot (one restart in the stats).  A record longer
    than slab + halo heads its slot and still does not fit: ENOMEM, after the earlier bytes were
    written."""
    from shock_amd import _lib as L
    S, H = 64 * KIB, 4 * KIB
    head = gen.fq_fill(3 * S - 1000)
    for name in NAMES:
        data = head + gen.fq_sized(50000, tag=3) + gen.fq_fill(2 * S + 333)
        p = tmp_path / "long.fq"
        p.write_bytes(data)
        out, n, err = oracle_lib.filter_fastq(data, name)
        r, got = _to_file(gpu_ctx, name, p, 0, len(data), tmp_path, slab_bytes=S, halo_bytes=H)
        assert r.status == L.OK and err is None and r.count == n and got == out
        assert gpu_ctx.filter_stats()["restarts"] == 1
        data = head + gen.fq_sized(S + H + 2000, tag=3) + gen.fq_fill(S)
        p.write_bytes(data)
        before, k, _ = oracle_lib.filter_fastq(head, name)
        r, got = _to_file(gpu_ctx, name, p, 0, len(data), tmp_path, slab_bytes=S, halo_bytes=H)
        assert r.status == L.ENOMEM and b"longer than a slab slot" in r.err
        assert r.count == k and got == before
    # gen.fastq's long records (35 to 70 KB of sequence, twice that per record) under slabs that hold them
    rng = random.Random(9)
    data = gen.fastq(rng, 400, long_every=150)
    p = tmp_path / "gen.fq"
    p.write_bytes(data)
    out, n, _ = oracle_lib.filter_fastq(data, "anonymize")
    r, got = _to_file(gpu_ctx, "anonymize", p, 0, len(data), tmp_path, slab_bytes=256 * KIB, halo_bytes=4 * KIB)
    assert r.status == L.OK and r.count == n and got == out


def test_stream_mirror(gpu_ctx, tmp_path):
    """filter.Stream: the Streamer's single-section case over an open file, Go's error after the bytes"""
    from shock_amd.filter import Stream
    from shock_amd.indexer import ShockIndexError
    p = tmp_path / "s.fq"
    p.write_bytes(b"@r1\nAC\n+\nII\n@r2\nA\n+\nIX\n")
    with open(p, "rb") as f, open(tmp_path / "o1", "wb") as w:
        with pytest.raises(ShockIndexError, match="length of sequence and quality"):
            Stream("fq2fa", f, w)
    assert (tmp_path / "o1").read_bytes() == b">r1\nAC\n"
    with open(p, "rb") as f, open(tmp_path / "o2", "wb") as w:
        assert Stream("anonymize", f, w, seek=0, length=12) == 11
    assert (tmp_path / "o2").read_bytes() == b"@1\nAC\n+\nII\n"
    with open(p, "rb") as f, open(tmp_path / "o3", "wb") as w, pytest.raises(KeyError):
        Stream("gzip", f, w)


# ---- under the cap -----------------------------------------------------------------------------
def test_filter_fd_under_the_cap(oracle_lib, tmp_path, shockidx_so):
    """A file of about 96 MiB under a 32 MiB device cap: shockidx_filter_fd takes the walk, delivers
    the oracle's bytes and holds no more than the cap; without a cap the same file takes the whole
    path with the same bytes.  A FASTA file that does not fit the cap under anonymize is ENOMEM with
    nothing written."""
    from shock_amd import Context, _lib as L
    block = gen.fastq(random.Random(77), 3000, plus_id=0.3)
    reps = (96 * MIB) // len(block) + 1
    data = block * reps
    p = tmp_path / "big.fq"
    p.write_bytes(data)
    ctx = Context(0)
    try:
        for name in NAMES:
            out, n, err = oracle_lib.filter_fastq(data, name)
            assert err is None
            ctx.set_dev_cap(32 * MIB)
            outp = tmp_path / "o.bin"
            with open(p, "rb") as f, open(outp, "wb") as w:
                r = ctx.filter_fd(name, f.fileno(), 0, len(data), w.fileno())
            st = ctx.filter_stats()
            assert r.status == L.OK and st["path"] == 2 and st["slabs"] > 3
            assert (r.count, r.size) == (n, len(out)) and outp.read_bytes() == out
            assert ctx.workspace_bytes() <= 32 * MIB and st["peak_bytes"] <= 32 * MIB
            ctx.set_dev_cap(0)
            with open(p, "rb") as f, open(outp, "wb") as w:
                r = ctx.filter_fd(name, f.fileno(), 0, len(data), w.fileno())
            assert r.status == L.OK and ctx.filter_stats()["path"] == 1
            assert (r.count, r.size) == (n, len(out)) and outp.read_bytes() == out
            ctx.trim(0)
        fa = gen.fasta(random.Random(3), 3000)
        assert len(fa) > 2 * MIB
        q = tmp_path / "f.fa"
        q.write_bytes(fa)
        ctx.set_dev_cap(32 * MIB)
        with open(q, "rb") as f, open(tmp_path / "o.fa", "wb") as w:
            r = ctx.filter_fd("anonymize", f.fileno(), 0, len(fa), w.fileno())
        assert r.status == L.ENOMEM and b"FASTA" in r.err and (tmp_path / "o.fa").read_bytes() == b""
        ctx.set_dev_cap(0)
        with open(q, "rb") as f, open(tmp_path / "o.fa", "wb") as w:  # it fits without the cap: the whole path
            r = ctx.filter_fd("anonymize", f.fileno(), 0, len(fa), w.fileno())
        out, n, err = oracle_lib.filter_fastq(fa, "anonymize")
        assert (r.status, r.err) == ((L.EFORMAT, err) if err else (L.OK, None))
        assert r.count == n and (tmp_path / "o.fa").read_bytes() == out
        nf = tmp_path / "none.txt"
        nf.write_bytes(b"hello world\n" * 10)
        with open(nf, "rb") as f, open(tmp_path / "o.n", "wb") as w:
            r = ctx.filter_fd("anonymize", f.fileno(), 0, 120, w.fileno())
        assert r.status == L.EFORMAT and r.err == b"Invalid file type for filter"
        assert (tmp_path / "o.n").read_bytes() == b""
    finally:
        ctx.close()
