"""bench.py: `--dump-outputs` (CPU: the writer; GPU: two plain runs of the same arguments dump the same arrays)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_arrays(tmp_path):
    out = {"reward": torch.linspace(-3.0, -1.0, 8), "actions": torch.arange(40).reshape(8, 5),
           "log_likelihood": torch.zeros(8, dtype=torch.float64), "grad_norm": None}
    bench.dump_outputs(out, None, False, str(tmp_path), torch)
    assert sorted(os.listdir(tmp_path)) == ["actions.npy", "log_likelihood.npy", "reward.npy"]
    a = np.load(tmp_path / "actions.npy")
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(40).reshape(8, 5))
    assert np.load(tmp_path / "log_likelihood.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "reward.npy"), out["reward"].numpy())


def test_dump_outputs_samples_the_same_rows_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    rows = 1000
    out = {"actions": torch.arange(rows * 4).reshape(rows, 4), "reward": -torch.arange(rows, dtype=torch.float32)}
    for d in ("a", "b"):
        bench.dump_outputs(out, None, False, str(tmp_path / d), torch)
    a, r = np.load(tmp_path / "a" / "actions.npy"), np.load(tmp_path / "a" / "reward.npy")
    assert a.nbytes + r.nbytes <= 4000 and a.shape[0] == r.shape[0] > 0
    assert np.array_equal(a[:, 0] / 4, -r)                       # one row sample shared by the arrays
    assert np.array_equal(a, np.load(tmp_path / "b" / "actions.npy"))     # and the same from run to run


@pytest.mark.gpu
def test_plain_bench_run_dumps_identical_outputs(tmp_path):
    """A plain run prints the contract keys only (no roofline / CPU baseline), and the same arguments dump the same arrays."""
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tsp20", "--steps", "3", "--warmup",
                            "1", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert "roofline" not in line and "cpu_baseline" not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert {"actions.npy", "reward.npy"} <= set(names) and names == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
