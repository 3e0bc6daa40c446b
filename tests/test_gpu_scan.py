"""GPU: the device-wide scans (sidx_scan.hpp, dscan::run) called directly, against exact integer
references in numpy (np.cumsum in uint64, shifted for the exclusive forms, and np.maximum.accumulate).

dscan::run has two implementations: inputs of up to sidx_scan_small_items() items take three plain
launches, larger ones the single-pass look-back kernel (tickets, flag words with a 62-bit payload, a
fold of 64 predecessors per step).  Through the public entry points only multi-GiB inputs leave the
small path, so every size here comes from the library's own constants: around one block, around 64
blocks (one fold of the look-back), around the switch between the two paths, and 65 blocks past it
(a second fold step).  All four instantiations in use run at every size: u32 -> u64 exclusive sum
(sidx_scan_flags), u64 exclusive sum (sidx_scan_u64), u64 exclusive max (sidx_scan_max_u64) and the
u64 inclusive sum behind sidx_crs_scan, whose input is a row table: k_crs_len takes each row's second
word as its length, and P[0] = 0, P[i + 1] = the sum of the first i + 1 lengths.

Every output is compared whole; the 64 words past it must keep their 0xAB fill (tests/kern.py)."""
import numpy as np
import pytest

import kern

pytestmark = pytest.mark.gpu

_U32MAX = (1 << 32) - 1


def _shape():
    return kern.scan_block(), kern.scan_small_items()


def _sizes():
    B, S = _shape()
    return [1, 7, 8, 9, 511, 512, 513, B - 1, B, B + 1, 64 * B - 1, 64 * B, 64 * B + 1, S - 1, S, S + 1, S + 65 * B + 3]


# the sizes as names (the values come from the library when the test runs)
SIZE_IDS = ["1", "7", "8", "9", "511", "512", "513", "B-1", "B", "B+1", "64B-1", "64B", "64B+1", "S-1", "S", "S+1",
            "S+65B+3"]


def _limit_vector(n):
    """Running total ending at exactly 2^62 - 1, the look-back payload's documented limit."""
    v = np.ones(n, np.uint64)
    v[0] = kern.PAY_MAX - (n - 1)
    return v


def _patterns(which, n, large):
    """[(name, values)]; at the largest sizes one or two patterns per entry point."""
    B, S = _shape()
    rng = np.random.default_rng(1000 + n % 9973)
    if which == "flags":
        pats = [("p0.5", rng.integers(0, 2, n, dtype=np.uint32)), ("all-2^32-1", np.full(n, _U32MAX, np.uint32))]
        if not large:
            pats += [("zeros", np.zeros(n, np.uint32)), ("ones", np.ones(n, np.uint32))]
        return pats
    if which == "u64":
        pats = [("below-2^40", rng.integers(0, 1 << 40, n, dtype=np.uint64))]
        if n in (B + 1, S + 1):
            pats.append(("total-2^62-1", _limit_vector(n)))
        return pats
    if which == "max":
        v = rng.integers(0, 1 << 61, n, dtype=np.uint64)
        v[rng.random(n) < 0.3] = 0  # the identity is 0: zeros must not disturb the maximum
        pats = [("non-monotone", v)]
        top = np.uint64(kern.PAY_MAX)
        # an exclusive scan never shows its last item: the spots lie before it.  The last item of the last
        # block that has a successor (inside one block: the item before the last), and the first item of
        # the last block that holds an item before the last
        last_of_block = ((n - 1) // B) * B - 1 if n > B else max(n - 2, 0)
        first_of_block = ((n - 2) // B) * B if n >= 2 else 0
        assert n < 2 or (last_of_block < n - 1 and first_of_block < n - 1)
        spots = [("max-at-0", 0), ("max-at-block-end", last_of_block), ("max-at-block-start", first_of_block)]
        for name, at in (spots[1:2] if large else spots):
            w = rng.integers(0, 1 << 40, n, dtype=np.uint64)
            w[at] = top
            pats.append((name, w))
        return pats
    rows = np.empty((n, 2), np.uint64)
    rows[:, 0] = rng.integers(0, 1 << 50, n, dtype=np.uint64)  # offsets: not part of the sums
    rows[:, 1] = rng.integers(0, 1 << 21, n, dtype=np.uint64)  # lengths around chunkrecord's 1 MiB limit
    rows[rng.random(n) < 0.2, 1] = 0
    pats = [("rows", rows)]
    if n in (B + 1, S + 1):
        lim = np.zeros((n, 2), np.uint64)
        lim[:, 0] = np.uint64((1 << 64) - 1)
        lim[:, 1] = _limit_vector(n)
        pats.append(("total-2^62-1", lim))
    return pats


@pytest.mark.parametrize("which", kern.SCANS)
@pytest.mark.parametrize("k", range(len(SIZE_IDS)), ids=SIZE_IDS)
def test_scan_exact_gpu(gpu_ctx, which, k):
    n = _sizes()[k]
    _, S = _shape()
    tmp = gpu_ctx.alloc(kern.scan_tmp_bytes(gpu_ctx, which, n))
    for name, values in _patterns(which, n, large=n >= S - 1):
        job = kern.ScanJob(gpu_ctx, which, values)
        assert job.launch(tmp) == kern.HIP_SUCCESS
        job.check(what=name)
        if which == "crs":
            ln = job.lengths()
            kern.first_diff(ln[:n], values[:, 1], f"crs lengths n={n} {name}")
            assert bool((ln[n:] == np.uint64(0xABABABABABABABAB)).all())
        job.free()
    tmp.free()


def test_scan_sizes_cover_both_paths_gpu(gpu_ctx):
    """The size query grows with the blocks, and the sizes above straddle the switch."""
    B, S = _shape()
    assert S % B == 0 and S // B >= 65 and B >= 513
    for which in kern.SCANS:
        q = [kern.scan_tmp_bytes(gpu_ctx, which, n) for n in (1, B, B + 1, S, S + 1)]
        assert q[0] == q[1] < q[2] < q[3] < q[4] and q[2] - q[1] == 8 and q[4] - q[3] == 8, (which, q)


@pytest.mark.parametrize("which", kern.SCANS)
def test_scan_short_workspace_gpu(gpu_ctx, which):
    """A workspace claimed one byte short is refused with hipErrorInvalidValue and nothing is scanned
    (sidx_crs_scan has by then cleared P[0] and copied the lengths; its sums stay untouched)."""
    B, S = _shape()
    ab = np.uint64(0xABABABABABABABAB)
    for n in (1, B + 1, S + 1):
        v = _patterns(which, n, large=True)[0][1]
        job = kern.ScanJob(gpu_ctx, which, v)
        tmp = gpu_ctx.alloc(job.need)
        assert job.launch(tmp, claim=job.need - 1) == kern.HIP_INVALID_VALUE
        got = job.result()
        assert bool((got[1 if which == "crs" else 0:] == ab).all()), (which, n)
        assert job.launch(tmp) == kern.HIP_SUCCESS  # the same buffers, now with the full size
        job.check(what="after the refusal")
        job.free()
        tmp.free()


@pytest.mark.parametrize("which", kern.SCANS)
def test_scan_empty_gpu(gpu_ctx, which):
    """n == 0: success, nothing written (sidx_crs_scan: P[0] = 0 alone)."""
    empty = {"flags": np.zeros(0, np.uint32), "crs": np.zeros((0, 2), np.uint64)}.get(which, np.zeros(0, np.uint64))
    job = kern.ScanJob(gpu_ctx, which, empty)
    tmp = gpu_ctx.alloc(job.need)
    assert job.launch(tmp) == kern.HIP_SUCCESS
    job.check(what="n=0")
    job.free()
    tmp.free()


def _back_to_back(ctx, plan):
    """plan: [(which, values)] launched in order on the context's stream with one workspace and no
    wait between them; every output exact."""
    jobs = [kern.ScanJob(ctx, which, v) for which, v in plan]  # uploads wait: all before the first launch
    tmp = ctx.alloc(max(j.need for j in jobs))
    rcs = [j.launch(tmp) for j in jobs]
    assert rcs == [kern.HIP_SUCCESS] * len(jobs)
    for i, j in enumerate(jobs):
        j.check(what=f"scan {i} of {len(jobs)} sharing a workspace")
        j.free()
    tmp.free()


@pytest.mark.parametrize("which", kern.SCANS)
def test_scan_workspace_reuse_gpu(gpu_ctx, which):
    """Look-back, small, look-back with different inputs: the small path leaves block prefixes where
    the look-back kernel keeps its ticket and flag words, and the next look-back must clear them."""
    B, S = _shape()
    plan = []
    for i, n in enumerate((S + 1, B + 1, S + 1)):
        pats = _patterns(which, n, large=True)
        v = pats[0][1].copy()
        if i == 2:  # a different input of the same size
            v = v[::-1].copy()
        plan.append((which, v))
    _back_to_back(gpu_ctx, plan)


@pytest.mark.parametrize("size", ["B+1", "S+1"])
def test_scan_max_then_sum_gpu(gpu_ctx, size):
    """The column index's pairing (and the FASTA boundaries'): a max scan, then a sum scan, one workspace."""
    B, S = _shape()
    n = B + 1 if size == "B+1" else S + 1
    mx = _patterns("max", n, large=True)[0][1]
    _back_to_back(gpu_ctx, [("max", mx), ("flags", _patterns("flags", n, True)[0][1]),
                            ("max", mx[::-1].copy()), ("u64", _patterns("u64", n, True)[0][1])])
