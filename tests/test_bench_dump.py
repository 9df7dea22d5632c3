"""`bench.py --dump-outputs DIR`: what the last timed step computed (loss sum, y_hat, the updated parameters) as .npy files,
identical from run to run with the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO


def test_dump_caps_large_arrays_with_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 400)
    big = torch.arange(1000, dtype=torch.float32)
    arrays = {"small": torch.tensor([1.5, -2.0]), "big": big, "wide": torch.arange(10, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b) and a.dtype == (np.float64 if name == "wide" else np.float32)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), [1.5, -2.0])
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.shape == (100,) and np.all(np.diff(s) > 0) and set(s.tolist()) <= set(big.tolist())


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--batch", "8", "--steps", "3",
                        "--warmup", "1", "--no-cpu-baseline", "--no-inference", "--no-configs", "--no-feed", "--no-p16",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_reproducibly(tmp_path):
    one, two = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    assert one["steps"] == 3 and one["ms_per_step"] > 0
    for name, shape in (("loss_sum", (1,)), ("y_hat", (8, 5, 10, 10)), ("params", (769349,))):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.shape == shape and a.dtype == np.float32 and np.isfinite(a).all(), name
        assert np.array_equal(a, b), name
    assert abs(float(np.load(tmp_path / "a" / "loss_sum.npy")[0]) - one["final_loss"]) <= 1e-4 * abs(one["final_loss"])
