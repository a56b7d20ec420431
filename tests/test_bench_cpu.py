"""bench.py's host-side pieces: --dump-outputs (file format, the 64 MB limit, the seeded sample) and the argument checks
that run before anything touches the GPU."""
import os
import subprocess
import sys

import numpy as np

import bench
from tests.conftest import ROOT


def _files(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_every_array_whole_when_it_fits(tmp_path):
    rng = np.random.default_rng(0)
    P, Q = rng.random((50, 8), np.float32), rng.random((30, 8), np.float32)
    bench.dump_outputs(str(tmp_path), {"P": P, "Q": Q})
    got = _files(tmp_path)
    assert sorted(got) == ["P.npy", "Q.npy"]
    assert got["P.npy"].dtype == np.float32 and np.array_equal(got["P.npy"], P) and np.array_equal(got["Q.npy"], Q)


def test_dump_outputs_samples_the_same_rows_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20_000)
    rng = np.random.default_rng(1)
    P, Q = rng.random((400, 16), np.float32), rng.random((100, 16), np.float32)  # 32 000 bytes of data
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"P": P, "Q": Q})
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert sorted(a) == ["P.npy", "P_rows.npy", "Q.npy", "Q_rows.npy"]
    assert all(np.array_equal(a[f], b[f]) for f in a)  # a fixed sample: the same rows every run
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_LIMIT_BYTES
    for name, full in (("P", P), ("Q", Q)):
        rows = a[f"{name}_rows.npy"]
        assert rows.dtype == np.float64 and 0 < rows.size < full.shape[0] and np.all(np.diff(rows) > 0)
        assert np.array_equal(a[f"{name}.npy"], full[rows.astype(np.int64)])


def test_bench_rejects_bad_arguments_before_it_starts():
    for args, msg in ((["--steps", "0"], "--steps must be at least 1"),
                      (["--gpus", "2", "--dump-outputs", "out"], "--dump-outputs: the single-GPU run only"),
                      (["--emulate-world", "4", "--dump-outputs", "out"], "--dump-outputs: the single-GPU run only")):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 2 and msg in p.stderr and p.stdout == "", (args, p.stderr)
