"""The download plan's host arithmetic (shock_amd/csrc/sidx_plan_host.hpp) on the CPU: the part
strings, SizePart in wrapping int64, the level-2 segment of a matrix record and the order of a
request's errors, tests/host/plan_test.cpp built as a stand-alone program with the host sanitizers
(ASan + UBSan) and run once.  No GPU, no library, no HIP call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")


def test_plan_host_program():
    subprocess.run(["make", "-s", "-C", CSRC, "plan_test"], check=True)
    p = subprocess.run([os.path.join(CSRC, "build", "plan_test")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert "plan_test ok" in p.stdout
    for report in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert report not in p.stdout, p.stdout
