"""The chunkrecord slab walk's arithmetic (shock_amd/csrc/sidx_chunkwalk.hpp) on the CPU: the slot
layout, slab sizing at and just under the smallest budget and never over a budget, the per-slab row
bound and the carry's precondition with its proof obligation (H >= WIN); tests/host/chunkwalk_test.cpp
built as a stand-alone program with the host sanitizers (ASan + UBSan) and run once.  Also: the header
declares the new entry points, the Python binding exports them, and the ABI version has not moved.
No GPU, no HIP call."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")
NEW = ("shockidx_chunkrecord_carry_bytes", "shockidx_chunkrecord_slab_device", "shockidx_chunkrecord_fd_walk")


def test_chunkwalk_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "chunkwalk_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "chunkwalk_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "chunkwalk_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout


def test_header_and_binding_have_the_chunk_slab_entry_points(shockidx_so):
    from shock_amd import _lib
    src = open(os.path.join(ROOT, "include", "shockidx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|uint64_t) %s\(" % name, code), name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name)
    assert "#define SHOCKIDX_ABI_VERSION 5" in src and _lib.lib().shockidx_abi_version() == 5
    # a header and two halves of (curr, off, count, format, done)
    assert _lib.lib().shockidx_chunkrecord_carry_bytes() >= 8 + 2 * 5 * 8


def test_context_has_the_chunk_slab_methods():
    from shock_amd import core
    for m in ("chunkrecord_carry", "chunkrecord_slab", "chunkrecord_fd_walk"):
        assert callable(getattr(core.Context, m))
