"""GPU: the format detection (sidx_control.hip: k_detect, k_detect_sections, det_skip and the three
matchers) at the edges of its 32768-byte window and of det_skip's 64-byte ballot steps, against
oracle.detect and pyref.detect_all (the literal regexes), which tests/test_oracle_anonymize.py shows to
agree on every input used here (tests/anonref.py).  A wrong answer silently changes which reader runs.

Context.detect cuts its input to the window, so every input also goes through
build_host(kind="record", fmt=None), where k_detect gets the full length: the format it reports and
Go's error must be the oracle's.  k_detect_sections is observed through the sectioned stream under
anonymize: a section that detects as nothing is "Invalid file type for filter" at its index."""
import numpy as np
import pytest

import anonref
import pyref
import streamref
from test_gpu_stream import _check as _stream_check

pytestmark = pytest.mark.gpu
NAMES = ("fasta", "fastq", "sam")


def _check(ctx, oracle, name, d):
    ofmt, omask = oracle.detect(d)
    assert [n for i, n in enumerate(NAMES) if omask >> i & 1] == pyref.detect_all(d), name
    assert ctx.detect(d) == (ofmt, omask), name
    r = ctx.build_host(d, kind="record", fmt=None)
    rows, err = oracle.record_index(d)
    assert r.fmt == ofmt and r.err == err and r.count == len(rows), (name, r.fmt, ofmt, r.err, err, r.count, len(rows))
    assert np.array_equal(r.rows if r.rows is not None else np.zeros((0, 2), np.uint64), rows), name
    return ofmt, omask


def test_detect_window_fasta_gpu(gpu_ctx, oracle_lib):
    """det_fasta's `i >= N` checks: the first sequence byte at offsets 32764..32767 matches, at 32768 it
    does not; 32764 leading '\\n' then ">a\\nA" ends on the window's last byte, 32765 '\\r' do not; k_detect's
    staging of the last 16-byte blocks of the window."""
    got = {name: _check(gpu_ctx, oracle_lib, name, d)[0] for name, d in anonref.det_window_fasta()}
    W = anonref.WINDOW
    assert [got[f"fasta-seq-at-{o}"] for o in range(W - 4, W + 1)] == ["fasta"] * 4 + [None]
    assert got["fasta-lead-nl-32764"] == "fasta" and got["fasta-lead-cr-32765"] is None


def test_detect_window_fastq_gpu(gpu_ctx, oracle_lib):
    """det_fastq's tail: `k == 0` (no newline after the plus line inside the window), `k >= 2` (an empty
    quality line: the second newline ends the match) and `k == 1` (\\S* then one more newline, which must
    lie inside the window: offsets 32765..32767 match, 32768 does not; without a final newline \\S* takes
    the zero padding and nothing follows)."""
    got = {name: _check(gpu_ctx, oracle_lib, name, d)[0] for name, d in anonref.det_window_fastq()}
    W = anonref.WINDOW
    assert [got[f"fastq-final-nl-at-{o}"] for o in range(W - 3, W + 1)] == ["fastq"] * 3 + [None]
    assert [got[f"fastq-empty-quality-2nd-nl-at-{o}"] for o in range(W - 2, W + 1)] == ["fastq"] * 2 + [None]
    assert got["fastq-empty-quality"] == "fastq" and got["fastq-one-nl-then-quality"] == "fastq"
    assert got["fastq-one-nl-then-space"] is None and got["fastq-no-final-newline"] is None


def test_detect_window_sam_gpu(gpu_ctx, oracle_lib):
    """det_sam's `e < N`: the terminating newline at 32766 and 32767 matches, at 32768 it does not."""
    got = {name: _check(gpu_ctx, oracle_lib, name, d)[0] for name, d in anonref.det_window_sam()}
    W = anonref.WINDOW
    assert [got[f"sam-nl-at-{o}"] for o in range(W - 2, W + 1)] == ["sam"] * 2 + [None]


def test_detect_ballot_steps_gpu(gpu_ctx, oracle_lib):
    """det_skip: every class run (leading newlines, ID and description, sequence, plus line, quality,
    the newline runs; FASTA's header and newline run; SAM's text) at 63, 64, 65, 127, 128 and 129 bytes,
    starting at offset 0 and 1 modulo 64 -- the run ends on the last lane of a ballot, on the first lane
    of the next, and one past it.  The byte after the run is the regex's next one (a match) or one that
    ends the match."""
    for name, d in anonref.det_ballot_steps():
        fmt, _ = _check(gpu_ctx, oracle_lib, name, d)
        assert (fmt is not None) == (not name.endswith("-after")), name


def test_detect_two_formats_gpu(gpu_ctx, oracle_lib):
    """det_match's mask and order (FASTA, then FASTQ, then SAM).  FASTQ + SAM is the only pair of the
    three anchored regexes that one input can match: FASTA wants '>' as the first byte after the
    newlines, FASTQ '@' and SAM one of [@[A-Z].  With FASTQ's last newline outside the window only SAM
    is left."""
    got = {name: _check(gpu_ctx, oracle_lib, name, d) for name, d in anonref.det_two_formats()}
    assert got["D1"] == ("fastq", 6) and got["D1-lead-nl"] == ("fastq", 6)
    assert got[f"fastq+sam-final-nl-at-{anonref.WINDOW - 1}"] == ("fastq", 6)
    assert got[f"fastq+sam-final-nl-at-{anonref.WINDOW}"] == ("sam", 4)


def test_detect_sections_gpu(gpu_ctx, oracle_lib):
    """k_detect_sections: the window-edge inputs as sections at pos % 16 in {0, 1, 7, 15} (the staging
    from 16-byte aligned loads, `p >= pos && p < hi`), each with its own length (m = min(len, 32768));
    sections of 1, 15, 16, 17 and 32767 bytes, whose padding DetBuf::at supplies without storing it;
    short sections followed in the node by the bytes that would complete their match (`p < hi` and
    `i < m`); the last section ending at a data_len that is no multiple of 16 (load16_partial).  Every
    section must show the result it gives alone (streamref's composition rule over the oracle)."""
    ok = lambda d: oracle_lib.filter_fastq(d, "anonymize")[2] is None  # noqa: E731
    nodes = anonref.det_section_nodes(ok)
    seen_none = 0
    for node, secs in nodes:
        assert len(secs) <= 40
        r = _stream_check(gpu_ctx, oracle_lib, "anonymize", node, secs)
        exp = streamref.stream_ref(oracle_lib, "anonymize", node, secs)
        assert r.err_section == exp[3] == (-1 if len(secs) > 4 else 1)
        seen_none += r.err == b"Invalid file type for filter"
    assert seen_none >= 40
