"""CPU: the generated nodes of tests/streamfmt.py against the oracle, so that the GPU tests of the
sectioned stream over FASTA and SAM sections (tests/test_gpu_stream_formats.py) cannot be vacuous: every
section of a passing node detects as the intended format and passes, every failing node fails at the
intended section with the intended text, and the numpy boundary reference of a FASTA section
(anonref.fasta_boundaries over the section's bytes alone) gives the oracle's delivered count."""
import numpy as np

import anonref
import streamfmt
import streamref


def _section_checks(oracle, name, fmt, data, secs, fail):
    for i, (pos, ln) in enumerate(secs):
        sec = data[pos:pos + ln]
        if fmt != "mixed":
            assert oracle.detect(sec)[0] == fmt, (name, i, sec[:40])
        out, count, err = oracle.filter_fastq(sec, "anonymize")
        if fail is not None and i == fail[0]:
            assert err is not None and err.startswith(fail[1]), (name, i, err)
        elif fail is None or i < fail[0]:
            assert err is None, (name, i, err)
        if fmt == "fasta" and err is None:
            assert count == len(anonref.fasta_boundaries(np.frombuffer(sec, np.uint8))), (name, i)
        if fmt == "sam" and err is None:
            lines = [l.strip() for l in sec.split(b"\n")[:-1]]  # ASCII trims: an upper bound otherwise
            assert count <= len(lines), (name, i)
    exp = streamref.stream_ref(oracle, "anonymize", data, secs)
    if fail is None:
        assert exp[2] is None and exp[3] == -1, (name, exp[2:])
    else:
        assert exp[3] == fail[0] and exp[2].startswith(fail[1]), (name, exp[2:], fail)


def test_subset_nodes(oracle_lib):
    for fmt, (data, secs) in (("fasta", streamfmt.fasta_subset()), ("sam", streamfmt.sam_subset())):
        assert len(secs) == 3000
        _section_checks(oracle_lib, f"{fmt}-subset", fmt, data, secs, None)
        exp = streamref.stream_ref(oracle_lib, "anonymize", data, secs)
        assert exp[1] > 3000 and len(exp[0]) > 100_000  # the stream is not empty


def test_edge_nodes(oracle_lib):
    nodes = streamfmt.edge_nodes(oracle_lib)
    assert sum(1 for n in nodes if n[4] is None) == 8  # a passing node per format and phase
    for name, fmt, data, secs, fail in nodes:
        _section_checks(oracle_lib, name, fmt, data, secs, fail)
        assert {p % 16 for p, _ in secs[:-1]} <= set(streamfmt.PHASES) and len(data) % 16 == 5
        for pos, ln in secs:
            assert data[pos - 1:pos] == b"\n"  # the byte before a section
    # what the edge sections are built for, per phase
    for ph in streamfmt.PHASES:
        for what, sec in streamfmt.fa_edge_sections(ph):
            b = anonref.fasta_boundaries(np.frombuffer(sec, np.uint8))
            if what.startswith(("nl|gt", "gt|gt", "gt-nl-gt", "nl-gt-gt")):
                e = {"lane": 80 - ph, "step": 1024 - ph, "step2": 2048 - ph}[what.rsplit("-", 1)[1]]
                assert (ph + e) % 16 == 0 and sec[e:e + 1] == b">"
                assert (e in b) == (not what.startswith("gt|gt")), (ph, what)
            if what == "nl-carried-3-steps":
                assert 4096 - ph + 5 in b
            if what == "gt-carried-3-steps":
                assert 100 in b and 4096 - ph + 5 not in b
        counts = {w: len(anonref.fasta_boundaries(np.frombuffer(s, np.uint8))) for w, s in streamfmt.fa_edge_sections(ph)}
        assert (counts["zero-boundaries"], counts["one-boundary"], counts["70-boundaries"]) == (0, 1, 70)


def test_rules_nodes(oracle_lib):
    nodes = streamfmt.rules_nodes(oracle_lib)
    assert sum(1 for n in nodes if n[4] is not None) >= 12
    for name, fmt, data, secs, fail in nodes:
        _section_checks(oracle_lib, name, fmt, data, secs, fail)
        assert max(ln for _, ln in secs) <= 1 << 20


def test_counter_and_failure_nodes(oracle_lib):
    data, secs = streamfmt.counter_node()
    out, count, err, esec = streamref.stream_ref(oracle_lib, "anonymize", data, secs)
    ids = [ln for ln in out.split(b"\n") if ln.startswith(b">")]
    assert err is None and count == 132 and ids == [b">%d" % (k + 1) for k in range(120)] + [b">%d" % (k + 1) for k in range(12)]
    for name, fmt, d, s, fail in streamfmt.first_failure_nodes():
        _section_checks(oracle_lib, name, fmt, d, s, fail)


def test_mixed_nodes(oracle_lib):
    data, secs, junk = streamfmt.alternating_node()
    fmts = [oracle_lib.detect(data[p:p + n])[0] for p, n in secs]
    assert fmts[:3] == ["fastq", "fasta", "sam"] and fmts[junk] not in ("fastq", "fasta", "sam")
    exp = streamref.stream_ref(oracle_lib, "anonymize", data, secs)
    assert (exp[2], exp[3]) == (streamfmt.TYPE_ERR, junk)
    data, secs = streamfmt.unaligned_batches_node()
    fmts = [oracle_lib.detect(data[p:p + n])[0] for p, n in secs]
    assert fmts == ["fastq"] * 5 + ["fasta"] * 3 + ["sam"] * 3
    sizes = [len(oracle_lib.filter_fastq(data[p:p + n], "anonymize")[0]) for p, n in secs]
    assert sum(sizes[:5]) % 2 == 1 and sum(sizes[:8]) % 16 != 0
