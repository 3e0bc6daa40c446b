"""GPU: the claim loop of the FASTQ and FASTA tile passes (k_fq_tiles, k_fa_tiles; the plan:
shock_amd/csrc/sidx_claim.hpp) against the oracle.

A workgroup takes its first claim of tiles by block index and every later one by a ticket of a
device counter, asked for some tiles ahead and handed to the workgroup's other waves through LDS.
What can go wrong is a tile run twice or never, a burst of tile words cut at the wrong place, a
ticket read before it arrived, a counter not reset between builds -- each would change the table,
the count or the error.  Contexts capped to a grid of three workgroups (debug_set_tiles_grid) put
every edge of the plan within a few MiB: with G = 3 the batch size B steps down from 32 to 2 where
the batches number fewer than 4 G = 12, i.e. at 24, 48, 96, 192 and 384 tiles, and the last three
batches are handed out in shorter claims."""
import contextlib
import random

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

TILE = 16384
GRID = 3
# tiles: the smallest files; one tile either side of every step of B at 4 G = 12 batches; a larger
# file whose last tile is short
SIZES = [1, 2, 3, 4, 23, 24, 25, 47, 48, 49, 95, 96, 97, 191, 192, 193, 383, 384, 385, 1000]
SHORT = 4321  # bytes of the last tile


@contextlib.contextmanager
def _capped(g=GRID):
    from shock_amd import Context
    ctx = Context(0)
    try:
        ctx.debug_set_tiles_grid(g)
        yield ctx
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def ctx3():
    with _capped() as ctx:
        yield ctx


def _nbytes(ntiles):
    return (ntiles - 1) * TILE + SHORT


_FA = {}


def _fasta(nbytes):
    """A valid FASTA of exactly nbytes: a generated block of records repeated, the last record's
    sequence stretched to the size."""
    if "base" not in _FA:
        _FA["base"] = gen.fasta(random.Random(41), 300, embedded_gt=0.1, crlf=0.1)
    base = _FA["base"]
    rep = base * (nbytes // len(base) + 1)
    k = rep.rfind(b"\n>", 0, max(nbytes - 8, 0))
    head = rep[:k + 1] if k >= 0 else b""
    tail = nbytes - len(head)
    assert tail >= 5, (nbytes, tail)
    out = head + b">t\n" + b"A" * (tail - 4) + b"\n"
    assert len(out) == nbytes
    return out


def _corpus(fmt, ntiles):
    n = _nbytes(ntiles)
    return gen.fq_fill(n) if fmt == "fastq" else _fasta(n)


_REF = {}


def _oracle(oracle_lib, fmt, ntiles):
    """(data, rows, err) of a corpus: computed once, shared by the cases that build it."""
    key = (fmt, ntiles)
    if key not in _REF:
        data = _corpus(fmt, ntiles)
        rows, err = oracle_lib.record_index(data, fmt)
        rows.setflags(write=False)
        _REF[key] = (data, rows, err)
    return _REF[key]


def _same(r, rows, err, what):
    assert r.count == len(rows), (what, r.count, len(rows), r.err, err)
    assert r.err == err, (what, r.err, err)
    got = r.rows if r.rows is not None else np.zeros((0, 2), np.uint64)
    if not np.array_equal(got, rows):
        bad = np.nonzero((got != rows).any(axis=1))[0][:5]
        raise AssertionError(f"{what}: first mismatching rows {bad.tolist()}: gpu {got[bad].tolist()} "
                             f"oracle {rows[bad].tolist()}")


def _build(ctx, oracle_lib, fmt, ntiles, auto=False):
    data, rows, err = _oracle(oracle_lib, fmt, ntiles)
    r = ctx.build_host(data, kind="record", fmt=None if auto else fmt)
    _same(r, rows, err, (fmt, ntiles))
    assert err is None
    return r


@pytest.mark.parametrize("ntiles", SIZES)
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_claim_sizes_grid3_gpu(ctx3, oracle_lib, fmt, ntiles):
    r = _build(ctx3, oracle_lib, fmt, ntiles)
    assert (r.path, r.reruns) == (1, 0), (fmt, ntiles, r.path, r.reruns)


@pytest.mark.parametrize("ntiles", [385, 1000])
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_claim_sizes_default_grid_gpu(gpu_ctx, oracle_lib, fmt, ntiles):
    r = _build(gpu_ctx, oracle_lib, fmt, ntiles)
    assert (r.path, r.reruns) == (1, 0), (fmt, ntiles, r.path, r.reruns)


def test_claim_set_grid_only_before_first_build_gpu(oracle_lib):
    from shock_amd._lib import ShockIdxError
    with _capped() as ctx:
        _build(ctx, oracle_lib, "fastq", 4)
        with pytest.raises(ShockIdxError):
            ctx.debug_set_tiles_grid(2)
    with pytest.raises(ShockIdxError):
        with _capped(0):
            pass


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_claim_counter_reset_between_builds_gpu(oracle_lib, fmt):
    """Two builds of different sizes on one context, both ways round: the second starts from ticket 0
    (a counter left at the first build's end would skip claims, or end the pass early)."""
    with _capped() as ctx:
        for ntiles in (193, 49, 385, 25):
            r = _build(ctx, oracle_lib, fmt, ntiles)
            assert (r.path, r.reruns) == (1, 0), (fmt, ntiles, r.path, r.reruns)


def test_claim_after_misspeculated_format_gpu(oracle_lib):
    """Auto-detecting builds run the format of the context's last build while k_detect decides: after
    a FASTQ build a FASTA file is first run, gated off, as FASTQ, and then again as FASTA."""
    with _capped() as ctx:
        _build(ctx, oracle_lib, "fastq", 97, auto=True)
        assert _nbytes(97) >= 1 << 20
        r = _build(ctx, oracle_lib, "fasta", 97, auto=True)
        assert r.fmt == "fasta"
        r = _build(ctx, oracle_lib, "fastq", 193, auto=True)
        assert r.fmt == "fastq"


def test_claim_after_format_error_gpu(oracle_lib):
    """A build that ends in a format error in the middle of the file, then a valid one."""
    data, _, _ = _oracle(oracle_lib, "fastq", 97)
    lines = data.split(b"\n")
    k = 4 * (len(lines) // 8) + 2  # a '+' line near the middle
    assert lines[k].startswith(b"+")
    lines[k] = b"-" + lines[k][1:]
    bad = b"\n".join(lines)
    rows, err = oracle_lib.record_index(bad, "fastq")
    assert err is not None and 0 < len(rows) < len(lines) // 4
    with _capped() as ctx:
        r = ctx.build_host(bad, kind="record", fmt="fastq")
        _same(r, rows, err, "mid-file error")
        r = _build(ctx, oracle_lib, "fastq", 49)
        assert (r.path, r.reruns) == (1, 0)


def test_claim_fq2fa_filter_gpu(ctx3, oracle_lib):
    """k_fq_tiles<true> (the filters' instantiation, which also keeps every record's line ends) takes
    the same loop."""
    data, _, _ = _oracle(oracle_lib, "fastq", 385)
    r = ctx3.filter_host("fq2fa", data)
    out, n, err = oracle_lib.filter_fastq(data, "fq2fa")
    assert r.status in (0, 1), (r.status, r.err)
    assert (r.count, r.err) == (n, err), (r.count, r.err, n, err)
    assert r.gathered == out
