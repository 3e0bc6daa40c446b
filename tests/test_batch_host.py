"""The batch build's host arithmetic (shock_amd/csrc/sidx_batch_host.hpp) on the CPU: the node range
check with its alignment and overflow cases, arena packing, the small-node limit, row regions and the
split into batched nodes and singles; tests/host/batch_test.cpp built as a stand-alone program with
the host sanitizers (ASan + UBSan) and run once.  Also the Python mirror's struct layouts and
CreateMany's argument checks.  No GPU, no HIP call."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")


def test_batch_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "batch_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "batch_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "batch_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout


def test_batch_structs_mirror_the_header(shockidx_so):
    from shock_amd import _lib
    src = open(os.path.join(ROOT, "include", "shockidx.h")).read()
    for struct, cls in (("shockidx_batch_item", _lib.BatchItem), ("shockidx_batch_stats", _lib.BatchStats)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"\b(\w+)(?:\[\d+\])?\s*;", body)
        assert names == [f[0] for f in cls._fields_], struct
    assert ctypes.sizeof(_lib.BatchItem) == 48 and ctypes.sizeof(_lib.BatchStats) == 10 * 8
    lib = _lib.lib()
    for name in ("shockidx_build_batch_device", "shockidx_build_batch_host", "shockidx_batch_error",
                 "shockidx_batch_last_stats"):
        assert name in _lib.EXPORTS and getattr(lib, name)


def test_create_many_checks_its_arguments():
    from shock_amd import indexer
    assert indexer.CreateMany([], []) == []
    with pytest.raises(ValueError):
        indexer.CreateMany([indexer.NewRecordIndexer(None)], [])
    with pytest.raises(ValueError):
        indexer.CreateMany([indexer.NewRecordIndexer(None), indexer.NewLineIndexer(None)], ["a", "b"])
    with pytest.raises(ValueError):
        indexer.CreateMany([indexer.NewChunkRecordIndexer(None)], ["a"])
    assert set(indexer.Indexers) == {"record", "line", "chunkrecord"}
