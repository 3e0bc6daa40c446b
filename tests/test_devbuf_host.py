"""The host bookkeeping (shock_amd/csrc/sidx_devbuf.hpp) on the CPU: the device-buffer set over a
malloc / free allocator and the error sink over both result structs, tests/host/devbuf_test.cpp
built as a stand-alone program with the host sanitizers (ASan + UBSan) and run once.  No GPU, no
library, no HIP call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")


def test_devbuf_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "devbuf_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "devbuf_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "devbuf_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout
