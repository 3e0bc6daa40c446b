"""The subset walk's arithmetic (shock_amd/csrc/sidx_subwalk.hpp) on the CPU: slab and window sizing
at and just under the smallest budget and never over a budget, the window after a stop at an id,
the rule for a line that heads a slot and the row and run cursors; tests/host/subwalk_test.cpp
built as a stand-alone program with the host sanitizers (ASan + UBSan) and run once.  Also: the
header declares the new entry points, the Python binding exports them, Context has the methods and
the ABI version has not moved.  No GPU, no HIP call."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")
NEW = ("shockidx_subset_carry_bytes", "shockidx_subset_slab_device", "shockidx_subset_fd_walk",
       "shockidx_subset_create", "shockidx_subset_last_stats")


def test_subwalk_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "subwalk_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "subwalk_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "subwalk_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout


def test_header_and_binding_have_the_subset_entry_points(shockidx_so):
    from shock_amd import _lib
    src = open(os.path.join(ROOT, "include", "shockidx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|uint64_t) %s\(" % name, code), name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name)
    assert "#define SHOCKIDX_ABI_VERSION 5" in src and _lib.lib().shockidx_abi_version() == 5
    for name in NEW:  # listed among the additions that did not move the version
        assert name in src[src.index("Added since without a version change"):src.index("#define SHOCKIDX_ABI_VERSION")]
    # the structs mirror the header's field for field
    for cname, cls in (("shockidx_subset_slab_result", _lib.SubsetSlabResult), ("shockidx_subset_stats", _lib.SubsetStats)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        fields = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
        assert fields == [f[0] for f in cls._fields_], (cname, fields)
    assert ctypes.sizeof(_lib.SubsetSlabResult) == 8 * 7 + 8 + 8 + 256 + 16
    assert 64 <= _lib.lib().shockidx_subset_carry_bytes() <= 256


def test_context_and_mirror_have_the_subset_methods():
    from shock_amd import core
    for m in ("subset_carry", "subset_slab", "subset_fd_walk", "subset_create", "subset_stats"):
        assert callable(getattr(core.Context, m))
