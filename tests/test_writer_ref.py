"""CPU: the reference of the direct writer tests (tests/test_gpu_filter_writer.py) is a composition --
the expected output of a row table is the concatenation, in row order, of the oracle's output of every
record delivered alone, under anonymize with its "@1\\n" replaced by "@<counter>\\n" (kern.record_ref).
Here that composition is proved equal to the oracle over the whole section with counters i + 1, for
both filters: on a generated corpus with CRLF and "+id" lines, and on the fixed-width constructed
records the writer tests build their 63-, 64- and 65-byte outputs from.

Every record used this way must be delivered alone (count == 1, no error); one that the standalone
format detection rejects -- a sequence ending in a Unicode space under anonymize -- is refused."""
import random

import pytest

import gen
import kern

NAMES = ("fq2fa", "anonymize")
MINIMAL = b"@a\nA\n+\nI\n"


def _split(oracle, data):
    rows, err = oracle.record_index(data, "fastq")
    assert err is None
    recs = [data[int(o):int(o) + int(n)] for o, n in rows]
    assert b"".join(recs) == data
    return recs


def _corpus():
    rng = random.Random(41)
    data = gen.fastq(rng, 300, crlf=0.3, plus_id=0.3)
    fixed = [gen.fq_rec(4, n, tag=t) for t, n in enumerate((57, 56, 58, 28, 27, 29, 1, 16))]
    fixed += [gen.fq_rec(3, 5, eol=b"\r\n"), gen.fq_rec(3, 5, plus_id=True), gen.fq_rec(2, 9, qual_at=True), MINIMAL]
    return data, b"".join(fixed * 25)


@pytest.mark.parametrize("name", NAMES)
def test_composition_equals_the_section(oracle_lib, name):
    for data in _corpus():
        recs = _split(oracle_lib, data)
        assert len(recs) == 300
        whole, count, err = oracle_lib.filter_fastq(data, name)
        assert (count, err) == (300, None)
        for r in recs:  # delivered alone
            out, c, e = oracle_lib.filter_fastq(r, name)
            assert c == 1 and e is None, (r[:40], c, e)
        parts = kern.section_ref(oracle_lib, name, recs)
        assert b"".join(parts) == whole


@pytest.mark.parametrize("name", NAMES)
def test_composition_with_long_records(oracle_lib, name):
    """Records longer than the detection's window ride behind a carrier in the reference: the same
    composition, proved on a section with such records first, in the middle, back to back and last."""
    rng = random.Random(42)

    def rec(nseq):
        return (b"@" + gen._word(rng, 1, 8) + b"\n" + gen._seq(rng, nseq, b"ACGTN") + b"\n+\n"
                + bytes(rng.randint(33, 74) for _ in range(nseq)) + b"\n")

    n = kern.DETECT_WINDOW
    recs = [MINIMAL, rec(n), rec(7), rec(n // 2), rec(n // 2 - 3), rec(3 * n + 5), rec(2 * n), MINIMAL, rec(n + 1)]
    assert sum(len(r) >= n for r in recs) == 6
    whole, count, err = oracle_lib.filter_fastq(b"".join(recs), name)
    assert (count, err) == (len(recs), None)
    assert b"".join(kern.section_ref(oracle_lib, name, recs)) == whole
    counters = [4294967296, 7, 100, 99999999, 1, 1000000000, 12, 5, 123456789]
    parts = kern.section_ref(oracle_lib, name, recs, counters)
    if name == "anonymize":
        assert [p.split(b"\n", 1)[0] for p in parts] == [b"@%d" % c for c in counters]
        assert b"".join(p.split(b"\n", 1)[1] for p in parts) == b"".join(
            p.split(b"\n", 1)[1] for p in kern.section_ref(oracle_lib, name, recs))


def test_fixed_width_outputs(oracle_lib):
    """The widths the staging-edge tests rely on: 64, 63 and 65 output bytes per record."""
    for nseq, want in ((57, 64), (56, 63), (58, 65)):
        assert len(kern.record_ref(oracle_lib, "fq2fa", gen.fq_rec(4, nseq), 1)) == want
    for nseq, counter, want in ((28, 10, 64), (28, 99, 64), (27, 100, 63), (27, 999, 63), (29, 1, 65), (29, 9, 65)):
        assert len(kern.record_ref(oracle_lib, "anonymize", gen.fq_rec(4, nseq), counter)) == want
    assert kern.record_ref(oracle_lib, "anonymize", MINIMAL, 4294967296) == b"@4294967296\nA\n+\nI\n"
    assert kern.record_ref(oracle_lib, "fq2fa", MINIMAL, 7) == b">a\nA\n"


def test_record_not_delivered_alone_is_refused(oracle_lib):
    uni = b"@r\nAC\xc2\xa0\n+\nII\n"  # the standalone detection answers "Invalid file type for filter"
    out, count, err = oracle_lib.filter_fastq(uni, "anonymize")
    assert count == 0 and err is not None
    with pytest.raises(AssertionError):
        kern.record_ref(oracle_lib, "anonymize", uni, 1)
    with pytest.raises(AssertionError):
        kern.record_ref(oracle_lib, "fq2fa", b"@r\nAC\n+\nI\n", 1)  # a length mismatch: an error, nothing delivered
