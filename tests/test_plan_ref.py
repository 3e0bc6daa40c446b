"""CPU: tests/planref.py, the reference of the download plan, against hand-derived vectors.

Reference: shock-server/controller/node/single.go:372-483 (the s.R = append(...) loops) over
node/file/index/index.go:67-193 and virtual.go:50-80.  The reference holds no tests or vectors for
this branch and no Go toolchain is available, so parity is unpinned by reference-held outputs:
planref composes the C restatements of Idx.Part / Idx.Range (pinned by tests/test_oracle_part.py)
the way the controller's loops do, and tests/golden/plan/kats.json holds known answers read off the
Go code line by line (cited per case).  This pins the composition rule, not Go itself.
"""
import json
import os

import numpy as np
import pytest

import planref

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan", "kats.json")))
MODES = {"PART": planref.PART, "RANGE": planref.RANGE, "CHUNK_RANGE": planref.CHUNK_RANGE, "SIZE": planref.SIZE}


def table(name):
    """a table of the fixture as uint64[k, 2] (None: the file is missing)"""
    if name is None:
        return None
    return np.array(KATS["tables"][name], dtype=np.int64).view(np.uint64).reshape(-1, 2)


def case_args(c):
    return (MODES[c["mode"]], c["parts"], table(c["rows"]), c["idx_length"], table(c["rec_rows"]), c["rec_length"],
            c["file_size"], c["chunk_size"])


def case_expect(c):
    return c["sections"], c["size"], (c["err"].encode() if c["err"] else None), c["err_part"]


@pytest.mark.parametrize("c", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_plan_kats(oracle_lib, c):
    assert planref.plan_ref(oracle_lib, *case_args(c)) == case_expect(c)


def test_fixture_holds_the_part_oracle_table():
    from test_oracle_part import ROWS
    assert np.array_equal(table("ROWS"), ROWS) and np.array_equal(table("ROWS3"), ROWS[:3])


def test_matrix_tables_are_what_the_chunkrecord_oracle_builds_for_short_chunks(oracle_lib):
    """MAT's rows have the matrix layout (16 * first row, 16 * rows), like the oracle's own output
    over the same record index (one chunk there: the records are far below 1 MiB)."""
    rec = table("REC")
    m = oracle_lib.chunkrecord_subset(rec)
    assert m.tolist() == [[0, 16 * len(rec)]]
    for c0, c1 in KATS["tables"]["MAT"]:
        assert c0 % 16 == 0 and c1 % 16 == 0 and c0 // 16 + c1 // 16 <= len(rec)


@pytest.mark.parametrize("part,size,chunk", [("1", 0, 5), ("0", 9, 5), ("+2", 9, 5), ("2-3-x", 20, 5), ("-1", 9, 5),
                                             ("3-1", 20, 5), ("9223372036854775807", 9, 2), ("2", 9, -(1 << 63))])
def test_size_part_wraps_like_int64(part, size, chunk):
    pos, ln, err = planref.size_part(part, size, chunk)
    for v in (pos, ln):
        assert -(1 << 63) <= v < (1 << 63)
    if part == "1":
        assert (pos, ln, err) == (0, 0, None)  # virtual.go:73: size - pos = 0 < 5
    if part == "0" or part == "-1":
        assert err is not None
    if part == "3-1":  # end < start is not rejected: fullReads = -10, 10 + 5 - 10 = 5 <= 20
        assert (pos, ln, err) == (10, -5, None)
