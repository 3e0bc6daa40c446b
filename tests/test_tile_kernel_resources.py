"""The register budget of the persistent tile kernels (k_fq_tiles<false>, k_fq_tiles<true>,
k_fa_tiles), read off the compiler's kernel resource report.  No GPU.

The tile loops keep no SlabParams field, 64-bit bound or thread predicate live from tile to tile
(sidx_kernels.hip, claim_loop "Registers"): the three kernels compile without one scalar or vector
register spilled and without scratch.  An edit that makes the compiler hoist such values again shows
here as spills, long before it shows in a benchmark.  The vector registers stay within what the grid
assumes: a kernel's workgroups per CU follow from its LDS block (hipOccupancyMaxActiveBlocksPer-
Multiprocessor sizes the grid), and with W workgroups of four waves per CU a wave may hold at most
512 / W registers, in steps of 8 -- 72 at 7 per CU (FASTQ), 64 at 8 per CU (FASTA).

sidx_kernels.hip is compiled for gfx950 with the Makefile's flags, device side only; the report is
the compiler's (-Rpass-analysis=kernel-resource-usage), no instruction is looked at."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shock_amd", "csrc")
LDS_PER_CU = 160 * 1024
KERNELS = {
    "k_fq_tiles<false>": "_ZN4sidx10k_fq_tilesILb0EEEvNS_10SlabParamsE",
    "k_fq_tiles<true>": "_ZN4sidx10k_fq_tilesILb1EEEvNS_10SlabParamsE",
    "k_fa_tiles": "_ZN4sidx10k_fa_tilesENS_10SlabParamsE",
}
FIELDS = {
    "vgprs": r"\bVGPRs: (\d+)",
    "agprs": r"\bAGPRs: (\d+)",
    "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
    "dynamic_stack": r"Dynamic Stack: (\w+)",
    "sgpr_spill": r"SGPRs Spill: (\d+)",
    "vgpr_spill": r"VGPRs Spill: (\d+)",
    "lds": r"LDS Size \[bytes/block\]: (\d+)",
}


def _makefile_vars():
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(HIPCC|ARCH|HIPFLAGS) \?= (.*)$", text, re.M)}
    assert set(var) == {"HIPCC", "ARCH", "HIPFLAGS"}, var
    return var


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """kernel symbol -> {field: value} for every kernel of sidx_kernels.hip: one compile."""
    var = _makefile_vars()
    hipcc = os.environ.get("HIPCC", var["HIPCC"])
    flags = var["HIPFLAGS"].replace("$(ARCH)", "gfx950").split()
    obj = tmp_path_factory.mktemp("res") / "sidx_kernels.o"
    cmd = [hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "sidx_kernels.hip"), "-o", str(obj)]
    p = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None or "remark:" not in line:
            continue
        for name, pat in FIELDS.items():
            m = re.search(pat, line)
            if m:
                cur[name] = m.group(1)
    return out


def _vgpr_budget(lds_bytes):
    """Registers a wave may hold with as many workgroups per CU as the LDS block lets in (at most 8:
    four waves each, 8 waves per SIMD)."""
    wgs = min(8, LDS_PER_CU // lds_bytes)
    return wgs, (512 // wgs) // 8 * 8


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_tile_kernel_has_no_spills(report, kernel):
    r = report.get(KERNELS[kernel])
    assert r is not None and set(r) == set(FIELDS), (kernel, r, sorted(report)[:8])
    print(kernel, r)
    assert int(r["sgpr_spill"]) == 0, (kernel, r)
    assert int(r["vgpr_spill"]) == 0, (kernel, r)
    assert int(r["scratch"]) == 0 and r["dynamic_stack"] == "False", (kernel, r)
    wgs, budget = _vgpr_budget(int(r["lds"]))
    assert wgs == (8 if kernel == "k_fa_tiles" else 7), (kernel, wgs, r)
    assert int(r["vgprs"]) + int(r["agprs"]) <= budget, (kernel, wgs, budget, r)
