"""The contract of the chunkrecord slab step, pinned against the reference's definition without the
library: a few-line slab walk over py_seek_chunk's window rule (test_oracle_chunk.py: fastq.go:216-243
/ fasta.go:143-173) with the carry (curr, off, first window = off == curr) equals py_chunkrecord for the
strides and cuts tests/test_gpu_chunk_slabs.py drives the device with.  A window that ends past a
view's end is io.EOF in the file's last view and "not here" in any other; nothing else crosses a slab
end.  CPU only."""
import random
import zlib

import numpy as np
import pytest

from test_oracle_chunk import WIN, fasta_records, fastq_records, py_chunkrecord, py_seek_chunk

STRIDES = (131072, 99984, 49152)
FRONTS = (65536, 32768)
CHUNKS = (WIN + 1, 40000, 65536)


def stride_views(n, stride, front):
    """Fixed-stride slabs as (lo, hi): slab k owns [k stride, (k + 1) stride) and reads `front` before it."""
    return [(max(0, b - front), min(n, b + stride)) for b in range(0, max(n, 1), stride)]


def cut_views(n, cuts):
    """Views that end at the given offsets (then at n); each starts as late as the carry allows: a walk
    stops only at a window with w > hi - WIN, so the next view may begin at hi - WIN + 1."""
    views, lo = [], 0
    for hi in list(cuts) + [n]:
        hi = min(hi, n)
        if views and hi <= views[-1][1]:
            continue
        views.append((lo, hi))
        lo = max(0, hi - WIN + 1)
    return views


def one_window(data, fmt, chunk, curr, off):
    """SeekChunk's window at offSet off of the chunk that starts at curr: the chunk length, or None."""
    w = off + chunk - WIN
    key = (fmt, w, off == curr)  # (a window's result depends on its bytes and lastIndex alone: kept per data)
    memo = _WINDOWS.setdefault(id(data), (data, {}))[1]
    if key not in memo:
        m, eof = py_seek_chunk(data[:w + WIN], fmt, chunk, off, off == curr)
        memo[key] = None if eof else m - (chunk - WIN)  # the match position in the window
    return None if memo[key] is None else (off - curr) + chunk - WIN + memo[key]


_WINDOWS = {}


def slab_walk_model(data, fmt, chunk, views):
    """-> (rows, rows per view, carries after each view as (curr, off, count, done))"""
    n, curr, off, done = len(data), 0, 0, False
    rows, per, carries = [], [], []
    for lo, hi in views:
        assert not done and off + chunk - WIN >= lo, "the carry's next window starts before the view"
        k0 = len(rows)
        while True:
            if off + chunk > hi:  # the window ends past the view
                if hi == n:
                    rows.append((curr, n - curr))
                    done = True
                break
            m = one_window(data, fmt, chunk, curr, off)
            if m is None:
                off += WIN
                continue
            rows.append((curr, m))
            curr += m
            off = curr
        per.append(len(rows) - k0)
        carries.append((curr, off, len(rows), done))
    return np.array(rows, dtype=np.uint64).reshape(-1, 2), per, carries


def make(fmt, variant, seed, size):
    rng = random.Random(seed)
    long = variant == "long"  # (records average about 9 KiB / 12 KiB then: fewer of them fill the size)
    if fmt == "fastq":
        data = fastq_records(rng, size // (4000 if long else 280) + 50, crlf=variant == "crlf",
                             at_qual=0.3 if variant == "atqual" else 0.0, long_every=12 if long else 0)
    else:
        data = fasta_records(rng, size // (5000 if long else 1500) + 20, crlf=variant == "crlf", long_every=6 if long else 0)
    return data[:size] if len(data) > size else data


def window_of_row(exp, k, chunk):
    """The start w of the window that closed chunk k of the table (its end lies in [w + 1, w + WIN - 1])."""
    curr, m = int(exp[k, 0]), int(exp[k, 1])
    j = (m - (chunk - WIN) - 1) // WIN  # windows without a match before it
    return curr + j * WIN + chunk - WIN


@pytest.mark.parametrize("fmt,variant", [("fastq", "plain"), ("fastq", "crlf"), ("fastq", "atqual"), ("fasta", "plain"),
                                         ("fasta", "crlf")])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_model_stride_sweep(fmt, variant, chunk):
    seed = zlib.crc32(f"{fmt}/{variant}/{chunk}".encode()) & 0xFFFF
    data = make(fmt, variant, seed, 300000 + seed % 200000)
    exp = py_chunkrecord(data, fmt, chunk)
    for stride in STRIDES:
        for front in FRONTS:
            rows, per, carries = slab_walk_model(data, fmt, chunk, stride_views(len(data), stride, front))
            assert np.array_equal(rows, exp), f"seed={seed} stride={stride} front={front}"
            assert sum(per) == len(exp) == carries[-1][2] and carries[-1][3]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_model_cuts_from_rows(fmt):
    chunk = 40000
    seed = zlib.crc32(f"cuts/{fmt}".encode()) & 0xFFFF
    data = make(fmt, "plain", seed, 400000)
    exp = py_chunkrecord(data, fmt, chunk)
    k = len(exp) // 2
    w = window_of_row(exp, k, chunk)
    for hi, closes in ((w + WIN, True), (w + WIN - 1, False), (w + 16, False)):
        views = cut_views(len(data), [hi])
        rows, per, carries = slab_walk_model(data, fmt, chunk, views)
        assert np.array_equal(rows, exp), f"seed={seed} hi={hi}"
        assert per[0] == (k + 1 if closes else k), (per, k)
        if not closes:
            assert carries[0][0] == int(exp[k, 0]) and views[1][0] <= w


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_model_mid_chunk_carry(fmt):
    """Windows without a match (records longer than a window): cuts after the first and the second
    unmatched window leave off > curr, once across two slab ends in a row."""
    chunk = WIN + 1
    seed = zlib.crc32(f"long/{fmt}".encode()) & 0xFFFF
    data = make(fmt, "long", seed, 600000)
    exp = py_chunkrecord(data, fmt, chunk)
    long_rows = [k for k in range(len(exp) - 1) if int(exp[k, 1]) >= 2 * WIN + 2]  # m - 1 = j WIN + pos, j >= 2
    assert long_rows, "no chunk with two unmatched windows"
    k = long_rows[0]
    w0 = int(exp[k, 0]) + chunk - WIN  # the chunk's first window
    for cuts in ([w0 + WIN], [w0 + 2 * WIN], [w0 + WIN, w0 + 2 * WIN]):
        rows, per, carries = slab_walk_model(data, fmt, chunk, cut_views(len(data), cuts))
        assert np.array_equal(rows, exp), f"seed={seed} cuts={cuts}"
        for c in carries[:len(cuts)]:
            assert c[1] > c[0] == int(exp[k, 0])  # mid-chunk: off past curr


def test_model_slabs_without_a_window():
    data = make("fastq", "plain", 5, 2500000)
    exp = py_chunkrecord(data, "fastq", 1 << 20)
    rows, per, carries = slab_walk_model(data, "fastq", 1 << 20, stride_views(len(data), 131072, 65536))
    assert np.array_equal(rows, exp) and per.count(0) > len(per) // 2
