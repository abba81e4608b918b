"""bench.py --dump-outputs: what the last timed step computed goes to DIR/*.npy in float32 / float64, exactly, within 64 MiB, and the same
cells every run, so that two builds can be compared output for output. CPU only: dump_outputs() on synthetic planes of the bench's shape."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_CELLS = 33289  # frave_amd.Plan(None, 4096, 4096, 1).num_cells: the bench's plane


def _plane(seed, cells=BENCH_CELLS):
    rng = np.random.default_rng(seed)
    co = rng.integers(-4096, 4096, size=(1, cells, 512), dtype=np.int32)
    co[rng.random(co.shape) < 0.01] = np.iinfo(np.int32).min  # None
    return co


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("coefs_sample", "coefs_sample_cells", "coefs_cell_sums")}


def test_bench_plane_size_matches_the_host_plan():
    import frave_amd

    assert frave_amd.Plan(None, 4096, 4096, 1).num_cells == BENCH_CELLS


def test_dump_is_exact_bounded_and_seeded(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    co = _plane(1)
    bench.dump_outputs(str(tmp_path / "a"), co)
    bench.dump_outputs(str(tmp_path / "b"), _plane(2))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "a")) == ["coefs_cell_sums.npy", "coefs_sample.npy", "coefs_sample_cells.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert a["coefs_sample"].dtype == np.float32 and a["coefs_sample_cells"].dtype == np.float64 and a["coefs_cell_sums"].dtype == np.float64
    cells = a["coefs_sample_cells"].astype(np.int64)
    assert len(cells) == bench.DUMP_SAMPLE_CELLS and np.all(np.diff(cells) > 0) and cells[-1] < BENCH_CELLS
    assert np.array_equal(cells, b["coefs_sample_cells"])  # the same cells whatever the plane holds
    assert np.array_equal(a["coefs_sample"].astype(np.int64), co[:, cells])
    assert np.array_equal(a["coefs_cell_sums"].astype(np.int64), co.sum(axis=2, dtype=np.int64))


def test_dump_of_a_small_plane_keeps_every_cell(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    co = _plane(3, cells=100)
    bench.dump_outputs(str(tmp_path), co)
    d = _load(tmp_path)
    assert np.array_equal(d["coefs_sample_cells"], np.arange(100)) and np.array_equal(d["coefs_sample"].astype(np.int64), co)


def test_bench_py_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--no-cpu-baseline"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout == ""
