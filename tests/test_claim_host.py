"""The tile passes' claim plan (shock_amd/csrc/sidx_claim.hpp) on the CPU: tests/host/claim_test.cpp
built as a stand-alone program with the host sanitizers (ASan + UBSan) and run once.  No GPU, no
library, no HIP call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")


def test_claim_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "claim_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "claim_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "claim_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout
