"""GPU: the sectioned stream over small FASTA and SAM sections under anonymize -- the segmented path of
sidx_stream.hip (k_ss_fa_count / k_ss_fa_emit / k_ss_sam_emit: a wave per section, 16 bytes per lane,
1 KiB per step) with the segmented forms of k_fa_anon_spans / k_fa_anon_write and the SAM kernels of
sidx_filter.hip on the flat rows.

The reference everywhere is streamref.stream_ref over the oracle plus the loop of filter_host over the
sections (test_gpu_stream._check); tests/test_stream_formats_ref.py pins the generated nodes
(tests/streamfmt.py) on the CPU.  Context.stream_stats() tells which path a call took."""
import numpy as np
import pytest

import anonref
import kern
import kern_stream
import streamfmt
import streamref
from shock_amd import _lib as L
from test_gpu_stream import _check, _device_call, _loop

pytestmark = pytest.mark.gpu


def _result(r):
    return (r.gathered, r.count, r.size, r.status, r.err, r.err_section)


def _run_node(ctx, oracle, node):
    name, fmt, data, secs, fail = node
    r = _check(ctx, oracle, "anonymize", data, secs)
    if fail is None:
        assert r.status == 0 and r.err_section == -1, (name, r.err, r.err_section)
    else:
        assert r.status == 1 and r.err_section == fail[0] and r.err.startswith(fail[1]), (name, r.err, r.err_section)
        # the bytes before the error are kept and nothing follows them
        kept = streamref.stream_ref(oracle, "anonymize", data, secs[:fail[0] + 1])[0]
        assert r.gathered == kept, name
    return r


# ---- 1. the path taken -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subset_refs(gpu_ctx, oracle_lib):
    """The reference of the two 3000-section lists, computed once: the composition rule over the oracle,
    which the per-section loop of filter_host has to reproduce."""
    refs = {}
    for fmt, (data, secs) in (("fasta", streamfmt.fasta_subset()), ("sam", streamfmt.sam_subset())):
        exp = streamref.stream_ref(oracle_lib, "anonymize", data, secs)
        assert _loop(gpu_ctx, "anonymize", data, secs) == exp
        refs[fmt] = exp
    return refs


@pytest.mark.parametrize("fmt", ["fasta", "sam"])
def test_path_taken_gpu(gpu_ctx, subset_refs, monkeypatch, fmt):
    """3000 small sections of one format are one batch; SHOCKIDX_STREAM_SMALL=0 sends every section
    through the single-section filter; a limit inside the lengths splits the list; the three streams are
    identical and equal the reference."""
    data, secs = streamfmt.fasta_subset() if fmt == "fasta" else streamfmt.sam_subset()
    exp = subset_refs[fmt]
    lens = sorted(n for _, n in secs)
    split = 300 if lens[0] <= 300 < lens[-1] else lens[len(lens) // 2]
    assert lens[0] <= split < lens[-1]
    got = {}
    for limit in (None, "0", str(split)):
        if limit is None:
            monkeypatch.delenv("SHOCKIDX_STREAM_SMALL", raising=False)
        else:
            monkeypatch.setenv("SHOCKIDX_STREAM_SMALL", limit)
        r = gpu_ctx.stream_filter_host("anonymize", data, secs)
        st = gpu_ctx.stream_stats()
        print(fmt, limit, st)
        assert st["sections"] == len(secs) and st["batched"] + st["singles"] == len(secs)
        if limit is None:
            assert (st["batches"], st["singles"]) == (1, 0)
            assert st["by_format"] == ([0, 1, 0] if fmt == "fasta" else [0, 0, 1])
        elif limit == "0":
            assert (st["batches"], st["batched"], st["singles"]) == (0, 0, len(secs))
        else:
            assert st["batches"] > 0 and st["singles"] > 0
            assert st["singles"] == sum(1 for n in lens if n > split)
        got[limit] = _result(r)
        assert (r.gathered, r.count, r.err, r.err_section) == exp and r.size == len(exp[0]) and r.status == 0
    assert got[None] == got["0"] == got[str(split)]


# ---- 2. section edges the wave walk can get wrong ------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_nodes(oracle_lib):
    return streamfmt.edge_nodes(oracle_lib)


def test_section_edges_gpu(gpu_ctx, oracle_lib, edge_nodes):
    for node in edge_nodes:
        _run_node(gpu_ctx, oracle_lib, node)
        if node[4] is None:
            st = gpu_ctx.stream_stats()
            assert st["singles"] == 0 and st["batches"] == 1, (node[0], st)


# ---- 3. the counter ------------------------------------------------------------------------------------------
def test_counter_restarts_gpu(gpu_ctx, oracle_lib):
    """120 sequences, then 12: >9, >10, >99, >100, then >1 again."""
    data, secs = streamfmt.counter_node()
    r = _check(gpu_ctx, oracle_lib, "anonymize", data, secs)
    ids = [ln for ln in r.gathered.split(b"\n") if ln.startswith(b">")]
    assert ids == [b">%d" % (k + 1) for k in range(120)] + [b">%d" % (k + 1) for k in range(12)]
    assert gpu_ctx.stream_stats()["by_format"] == [0, 1, 0]


# ---- 4. Read's rules inside small sections -------------------------------------------------------------------
def test_read_rules_gpu(gpu_ctx, oracle_lib):
    nodes = streamfmt.rules_nodes(oracle_lib)
    for node in nodes:
        _run_node(gpu_ctx, oracle_lib, node)
        st = gpu_ctx.stream_stats()
        assert st["singles"] == 0, (node[0], st)  # every section is under the limit


# ---- 5. the first failure --------------------------------------------------------------------------------------
def test_first_failure_gpu(gpu_ctx, oracle_lib):
    for node in streamfmt.first_failure_nodes():
        r = _run_node(gpu_ctx, oracle_lib, node)
        assert r.err_section == node[4][0]
        assert gpu_ctx.stream_stats()["singles"] == 0


# ---- 6. mixed lists --------------------------------------------------------------------------------------------
def test_mixed_formats_gpu(gpu_ctx, oracle_lib):
    data, secs, junk = streamfmt.alternating_node()
    r = _check(gpu_ctx, oracle_lib, "anonymize", data, secs)
    assert (r.err, r.err_section) == (streamfmt.TYPE_ERR, junk)
    st = gpu_ctx.stream_stats()
    # a batch per section (the format changes at every one), the junk section alone
    assert st["singles"] == 1 and st["batches"] == len(secs) - 1 and st["by_format"] == [4, 3, 3], st
    _check(gpu_ctx, oracle_lib, "anonymize", data, secs[:junk])
    assert gpu_ctx.stream_stats()["by_format"] == [3, 3, 3]


def test_unaligned_batches_gpu(gpu_ctx, oracle_lib):
    data, secs = streamfmt.unaligned_batches_node()
    _check(gpu_ctx, oracle_lib, "anonymize", data, secs)
    st = gpu_ctx.stream_stats()
    assert (st["batches"], st["batched"], st["by_format"]) == (3, len(secs), [1, 1, 1]), st
    _check(gpu_ctx, oracle_lib, "anonymize", data, secs[5:] + secs[:5])  # FASTA first, SAM and FASTQ staged


def test_overlapping_repeated_reversed_gpu(gpu_ctx, oracle_lib):
    data, secs = streamfmt.fasta_subset()
    s = secs[:40]
    over = [(s[i][0], s[i + 1][0] + s[i + 1][1] - s[i][0]) for i in range(0, 20)]  # each overlaps the next
    _check(gpu_ctx, oracle_lib, "anonymize", data, over + [s[3]] * 3 + s[::-1])
    data, secs = streamfmt.sam_subset()
    s = secs[:40]
    _check(gpu_ctx, oracle_lib, "anonymize", data, s[::-1] + [s[5], s[5]] + [(s[2][0], s[4][0] - s[2][0])])


# ---- 7. capacity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fasta-one-batch", "sam-one-batch", "several-groups"])
def test_capacity_gpu(gpu_ctx, oracle_lib, which):
    if which == "fasta-one-batch":
        data, secs = streamfmt.fasta_subset()
        secs = secs[:200]
    elif which == "sam-one-batch":
        data, secs = streamfmt.sam_subset()
        secs = secs[:200]
    else:
        data, secs = streamfmt.unaligned_batches_node()
    exp = streamref.stream_ref(oracle_lib, "anonymize", data, secs)
    size = len(exp[0])
    assert exp[2] is None and size > 64
    r, d_in, d_secs, d_out = _device_call(gpu_ctx, "anonymize", data, secs, size - 1)
    assert r.status == L.ESPACE and r.size == size, (r.status, r.size, size)
    assert bytes(d_out.download(size + 63)) == b"\xab" * (size + 63)  # nothing written
    assert (gpu_ctx.stream_stats()["batches"] > 1) == (which == "several-groups")
    r = gpu_ctx.stream_filter_device("anonymize", d_in.ptr, len(data), d_secs.ptr, len(secs), d_out.ptr, size)
    assert (r.status, r.size, r.count, r.err_section) == (0, size, exp[1], -1)
    got = d_out.download(size + 63).tobytes()
    assert got[:size] == exp[0] and got[size:] == b"\xab" * 63  # exact capacity: the bytes past the output stay
    for b in (d_in, d_secs, d_out):
        b.free()


# ---- 8. direct launches ----------------------------------------------------------------------------------------
def _job(ctx, fmt, data, secs, what):
    job = kern_stream.IndexJob(ctx, fmt, np.frombuffer(data, np.uint8) if isinstance(data, bytes) else data, secs)
    try:
        return job.check(what)
    finally:
        job.free()


def test_index_kernels_edge_nodes_gpu(gpu_ctx, edge_nodes):
    total = 0
    for name, fmt, data, secs, fail in edge_nodes:
        total += _job(gpu_ctx, fmt, data, secs, name)
    assert total > 500


@pytest.mark.parametrize("fmt", ["fasta", "sam"])
def test_index_kernels_random_gpu(gpu_ctx, fmt):
    """2000 random sections (lengths 0 to 5000, any alignment, overlapping) of bytes heavy in '>' and
    '\\n', and the whole buffer cut at the carry cases' 1 KiB and 16-byte edges."""
    data = anonref.bnd_random(3)
    rng = np.random.default_rng(77)
    pos = rng.integers(0, len(data) - 5000, 2000)
    ln = rng.integers(0, 5000, 2000)
    ln[:50] = rng.integers(0, 40, 50)
    secs = np.stack([pos, ln], axis=1)
    secs[-1] = (len(data) - 777, 777)  # ends at data_len
    K = _job(gpu_ctx, fmt, data, secs, f"random-{fmt}")
    assert K > 100_000
    for name, buf in anonref.bnd_carry_cases()[:4]:
        cuts = [(0, len(buf)), (1, len(buf) - 1), (15, 3 * 1024 + 1), (100, len(buf) - 100), (101, 1), (16, 0)]
        _job(gpu_ctx, fmt, buf, cuts, name)


# ---- 9. the Python mirror --------------------------------------------------------------------------------------
def test_streamer_mirror_fasta_gpu(gpu_ctx, oracle_lib):
    from shock_amd import Streamer
    from shock_amd.indexer import ShockIndexError
    name, fmt, data, secs, fail = streamfmt.first_failure_nodes()[0]
    exp = streamref.stream_ref(oracle_lib, "anonymize", data, secs)
    s = Streamer(R=secs, Filter="anonymize")
    rd = s.Stream(data)
    assert rd.read(len(exp[0])) == exp[0]
    with pytest.raises(ShockIndexError, match="Invalid fasta entry"):
        rd.read()
    assert s.ESection == fail[0] and "Invalid fasta entry" in str(s.E)
    data, secs = streamfmt.counter_node()
    s = Streamer(R=secs, Filter="anonymize")
    assert s.Stream(data).read() == streamref.stream_ref(oracle_lib, "anonymize", data, secs)[0] and s.E is None
