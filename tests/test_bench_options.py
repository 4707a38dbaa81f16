"""bench.py's command line without a GPU: the options exist, --steps is checked before anything starts, and --dump-outputs keeps under its size limit."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_options():
    p = _run("--help")
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = _run("--steps", "0")
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr


def test_dump_outputs_whole(tmp_path):
    x = np.arange(24, dtype=np.float64).reshape(4, 3, 2)
    status = np.array([0, 1, 0, 0], dtype=np.int32)
    bench.dump_outputs(str(tmp_path), {"x": x, "status": status})
    assert sorted(os.listdir(tmp_path)) == ["status.npy", "x.npy"]
    assert np.array_equal(np.load(tmp_path / "x.npy"), x)
    s = np.load(tmp_path / "status.npy")
    assert s.dtype == np.float64 and np.array_equal(s, status)


def test_dump_outputs_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 1000.0)
    x = np.random.default_rng(1).standard_normal((400, 5))
    loss = x.sum(axis=1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "loss": loss})
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["loss.npy", "loss_rows.npy", "x.npy", "x_rows.npy"]
    assert sum(np.load(a / f).nbytes for f in ("x.npy", "loss.npy")) <= 8 * 1000
    for f in os.listdir(a):                                     # the sample is fixed: the same rows every run
        assert np.array_equal(np.load(a / f), np.load(b / f))
    rows = np.load(a / "x_rows.npy").astype(int)
    assert np.array_equal(np.load(a / "x.npy"), x[rows]) and np.array_equal(np.load(a / "loss_rows.npy").astype(int), rows)
    assert np.array_equal(np.load(a / "loss.npy"), loss[rows])
