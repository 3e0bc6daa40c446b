"""CPU: the composition rule of the sectioned stream (tests/streamref.py) against hand-written known
answers (tests/golden/stream/kats.json): the anonymize counter restarts in every section, a record cut
by a section end in the middle of the list is dropped without an error, the stream stops after the
first failing section and keeps that section's bytes, and an empty section is a detection failure under
anonymize and nothing under fq2fa (request/streamer.go:78-98 over node/filter/)."""
import pytest

import streamref

KATS = streamref.load_kats()


def test_kats_cover_the_rule():
    ids = {k[0] for k in KATS}
    assert len(KATS) >= 10 and len(ids) == len(KATS)
    assert {"counter_restart", "mid_list_eof_drop", "stop_at_first_failing", "empty_section_fq2fa",
            "empty_section_anonymize"} <= ids


@pytest.mark.parametrize("kat", KATS, ids=[k[0] for k in KATS])
def test_stream_ref_kat(oracle_lib, kat):
    _, name, data, secs, out, esec, err = kat
    got_out, _, got_err, got_esec = streamref.stream_ref(oracle_lib, name, data, secs)
    assert (got_out, got_err, got_esec) == (out, err, esec)


def test_stream_ref_counts_and_whole_section(oracle_lib):
    """One section over the whole buffer is the single-section filter; counts add up over sections."""
    data = b"@a\nAC\n+\nII\n@b\nG\n+\nJ\n"
    for name in ("fq2fa", "anonymize"):
        o, n, e = oracle_lib.filter_fastq(data, name)
        assert streamref.stream_ref(oracle_lib, name, data, [(0, len(data))]) == (o, n, e, -1)
        assert streamref.stream_ref(oracle_lib, name, data, [(0, 11), (11, 9), (0, 20)])[1] == 4
