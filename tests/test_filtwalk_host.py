"""The download filters' slab walk arithmetic (shock_amd/csrc/sidx_filtwalk.hpp) on the CPU: slab sizing
at and just under the smallest budget and never over a budget, slab positions, the row cap against a
slab of shortest records, the output bound at counters of 1, 8, 9 and 20 digits and the restart /
ENOMEM decision; tests/host/filtwalk_test.cpp built as a stand-alone program with the host sanitizers
(ASan + UBSan) and run once.  Also: the header declares the new entry points, the Python binding
exports them, the Context methods exist and the ABI version has not moved.  No GPU, no HIP call."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")
NEW = ("shockidx_filter_carry_bytes", "shockidx_filter_slab_device", "shockidx_filter_fd_walk",
       "shockidx_filter_fd", "shockidx_filter_last_stats")


def test_filtwalk_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "filtwalk_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "filtwalk_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "filtwalk_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout


def test_header_and_binding_have_the_filter_slab_entry_points(shockidx_so):
    from shock_amd import _lib
    src = open(os.path.join(ROOT, "include", "shockidx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|uint64_t) %s\(" % name, code), name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name)
        assert name in src[:src.index("#define SHOCKIDX_ABI_VERSION")], name  # the list of additions
    assert re.search(r"\}\s*shockidx_filter_stats;", code)
    assert "#define SHOCKIDX_ABI_VERSION 5" in src and _lib.lib().shockidx_abi_version() == 5
    # the binding's mirrors: nine u64 words of stats; the carry is a header and two halves
    fields = re.search(r"typedef struct shockidx_filter_stats \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", fields) == [k for k, _ in _lib.FilterStats._fields_]
    assert _lib.lib().shockidx_filter_carry_bytes() == ctypes.sizeof(_lib.FilterCarry) == 192


def test_context_has_the_filter_slab_methods():
    from shock_amd import core, filter as flt
    for m in ("filter_carry", "filter_slab", "filter_fd_walk", "filter_fd", "filter_stats"):
        assert callable(getattr(core.Context, m))
    assert callable(flt.Stream)
