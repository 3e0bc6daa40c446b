"""bench.py's command line: a plain run does the timed steps only, --full adds the parity check,
the streaming floor, the CPU baseline and the PMC lookup; --dump-outputs writes the last build's
record count and a fixed sample of its row table as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_skips_everything_beside_the_steps(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup) == (7, 2)
    assert not a.full and not a.check and not a.floor and a.cpu_sec == 0 and a.dump_outputs is None


def test_full_keeps_the_side_measurements_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and a.check and a.floor and a.cpu_sec == 10.0
    a = _parse(monkeypatch, "--full", "--no-check", "--no-floor", "--cpu-sec", "0")
    assert a.full and not a.check and not a.floor and a.cpu_sec == 0


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1"), ("--gpus", "2", "--dump-outputs", "d"),
                                  ("--e2e", "--dump-outputs", "d"), ("--kind", "filter", "--dump-outputs", "d")])
def test_refused_arguments(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


class _Rows:
    """Stands in for the device row table: row i = (100 i, 100)."""

    def rows(self, count):
        i = np.arange(count, dtype=np.uint64)
        return np.stack([100 * i, np.full(count, 100, dtype=np.uint64)], axis=1)


@pytest.mark.parametrize("count", [0, 5, (1 << 19) + 3, 3_000_000])
def test_dump_outputs_sample(tmp_path, count):
    import bench
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _Rows(), count)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["count.npy", "rows_sample.npy", "rows_sample_ids.npy"]
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:  # float64, and the same sample from call to call
        assert got[n].dtype == np.float64 and np.array_equal(got[n], np.load(tmp_path / "b" / n))
    ids, tab = got["rows_sample_ids.npy"], got["rows_sample.npy"]
    assert got["count.npy"].tolist() == [count]
    assert tab.shape == (len(ids), 2) and np.array_equal(tab[:, 0], 100 * ids) and np.all(tab[:, 1] == 100)
    assert np.all(np.diff(ids) > 0) and (count == 0 or (ids[0] == 0 and ids[-1] == count - 1))
    edge = min(count, bench.DUMP_EDGE)
    assert np.array_equal(ids[:edge], np.arange(edge)) and np.array_equal(ids[len(ids) - edge:], np.arange(count - edge, count))
    if count <= 2 * bench.DUMP_EDGE:
        assert len(ids) == count  # a small table is written whole
    # whatever the table's size, the files stay under 64 MB: 24 bytes per sampled row
    assert 24 * (2 * bench.DUMP_EDGE + bench.DUMP_DRAW) + 3 * 128 + 8 < 64e6
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 24 * len(ids) + 3 * 128 + 8


@pytest.mark.gpu
def test_plain_bench_dumps_what_it_built(tmp_path):
    """A plain run on a 48 MiB file: the steps asked for, ms_per_step, none of --full's keys, and a
    dump whose rows tile the file from offset 0 (the table is small enough to be written whole)."""
    size_gib = 48 / 1024
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size-gib", str(size_gib), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert "cpu_baseline" not in line and "box_floor" not in line and line["parity"]["rows_checked"] == 0
    count = line["config"]["records"]
    ids, tab = np.load(tmp_path / "out" / "rows_sample_ids.npy"), np.load(tmp_path / "out" / "rows_sample.npy")
    assert np.load(tmp_path / "out" / "count.npy").tolist() == [count] and line["parity"]["count_ok"]
    assert np.array_equal(ids, np.arange(count)) and tab.dtype == np.float64
    assert tab[0, 0] == 0 and np.array_equal(tab[1:, 0], tab[:-1, 0] + tab[:-1, 1])
    size = int(size_gib * (1 << 30))
    # whole records only, '\n' padding after the last: a synthetic FASTQ record is 125 (synth.MIN_REC) to
    # 630 bytes (sidx_synth.hip fq_rec: two lines of at most 251, two id lines of at most 64)
    assert size - 630 < tab[-1, 0] + tab[-1, 1] <= size and np.all((tab[:, 1] >= 125) & (tab[:, 1] <= 630))
