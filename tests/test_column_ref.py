"""CPU: the column index's Python restatement (tests/colref.py, written from index/column.go)
against its known answers, its loop form against the closed form the device build computes, and
the C header's two column entry points."""
import json
import os
import random
import re

import colref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "column", "kats.json")))


def _kat_data(k):
    if "fixture" in k:
        return open(os.path.join(ROOT, "tests", "golden", "fixtures", k["fixture"]), "rb").read()
    return k["data"].encode("latin-1")


def test_known_answers():
    assert len(KATS) >= 18
    for k in KATS:
        r = colref.column_index(_kat_data(k), k["column"])
        assert r[0] == k["status"], k
        if r[0] == "ok":
            assert [list(x) for x in r[1]] == k["rows"], k


def test_issue_answers_literal():
    """The six answers the feature was specified with, spelled out (not read from the file)."""
    for data, c, rows in ((b"\n\nx\t1\nx\t2\n", 1, [(0, 2), (2, 8)]), (b"x\ty\nx\ty", 2, [(0, 4), (4, 3)]),
                          (b"a\n", 1, []), (b"", 1, []), (b"a\nb", 1, []), (b"a\nbb", 1, [(0, 2), (2, 2)])):
        assert colref.column_index(data, c) == ("ok", rows)
        assert colref.closed_form(data, c) == ("ok", rows)


def test_loop_form_equals_closed_form():
    rng = random.Random(20240611)
    alphabet = b"ab\t\n\r"
    seen = {"ok": 0, "err": 0, "panic": 0}
    for _ in range(20000):
        data = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 24)))
        c = rng.randint(1, 4)
        r = colref.column_index(data, c)
        seen[r[0]] += 1
        want = ("err",) if r[0] == "panic" else r
        assert colref.closed_form(data, c) == want, (data, c, r)
        if r[0] == "ok" and r[1]:  # contiguous, non-empty rows covering the file
            assert r[1][0][0] == 0 and sum(n for _, n in r[1]) == len(data)
            assert all(n > 0 for _, n in r[1])
            assert all(a[0] + a[1] == b[0] for a, b in zip(r[1], r[1][1:]))
    assert all(seen.values()), seen


def test_header_declares_column_entry_points():
    src = open(os.path.join(ROOT, "include", "shockidx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(shockidx_[a-z_]+)\s*\(", src))
    assert {"shockidx_column_device", "shockidx_column_fd"} <= names
    assert "#define SHOCKIDX_ABI_VERSION 5" in src


def test_python_surface():
    from shock_amd import indexer
    from shock_amd.core import Context
    for m in ("column_device", "column_fd", "column_buffer", "column_host"):
        assert callable(getattr(Context, m))
    assert callable(indexer.NewColumnIndexer) and callable(indexer.CreateColumnIndex)
    assert "column" not in indexer.Indexers  # controller/node/index/index.go:176: not a registry key
