"""The column slab walk's arithmetic (shock_amd/csrc/sidx_colwalk.hpp) on the CPU: slab sizing at and
just under the smallest budget and never over a budget, the slot layout, the one retry rule and the
row cursor; tests/host/colwalk_test.cpp built as a stand-alone program with the host sanitizers
(ASan + UBSan) and run once.  Also: the header declares the new entry points, the Python binding
exports them, and the ABI version has not moved.  No GPU, no HIP call."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")
NEW = ("shockidx_column_carry_bytes", "shockidx_column_slab_device", "shockidx_column_fd_walk",
       "shockidx_column_create")


def test_colwalk_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "colwalk_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "colwalk_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "colwalk_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout


def test_header_and_binding_have_the_slab_entry_points(shockidx_so):
    from shock_amd import _lib
    src = open(os.path.join(ROOT, "include", "shockidx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|uint64_t) %s\(" % name, code), name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name)
    # the fifth new symbol is the return code
    assert re.search(r"\bSHOCKIDX_EMORE = 2\b", code) and _lib.EMORE == 2
    assert re.search(r"#define SHOCKIDX_COLUMN_KEYCAP (\d+)", code).group(1) == str(_lib.COLUMN_KEYCAP) == "65536"
    assert "#define SHOCKIDX_ABI_VERSION 5" in src and _lib.lib().shockidx_abi_version() == 5
    assert _lib.lib().shockidx_column_carry_bytes() >= 64 + _lib.COLUMN_KEYCAP


def test_context_has_the_slab_methods():
    from shock_amd import core
    for m in ("column_slab", "column_carry", "column_fd_walk", "column_create"):
        assert callable(getattr(core.Context, m))
