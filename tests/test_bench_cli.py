"""bench.py's command line: `--dump-outputs` (what the last timed step returned, as .npy) and the plain / `--full` split."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float32_whole_when_small(tmp_path):
    t = torch.randn(2, 16, 8).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path), {"image_features": t})
    a = np.load(tmp_path / "image_features.npy")
    assert a.dtype == np.float32 and a.shape == (2, 16, 8)
    assert np.array_equal(a, t.float().numpy())


def test_dump_outputs_samples_a_fixed_subset_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 1000)
    t = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": t})
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.dtype == np.float32 and a.size == 1000 and a.nbytes <= 4 * 1000
    assert np.array_equal(a, b)                              # the same elements every run
    assert np.all(np.diff(a) > 0)                            # ascending flat indices of distinct elements


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    return r


def test_steps_below_one_is_refused():
    r = _bench("--steps", "0")
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_carries_only_the_headline(tmp_path):
    r = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--res", "256", "--dump-outputs", str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "images/sec" and d["dtype"] == "bf16"
    assert not {"roofline", "kernels", "power", "ttft", "cpu_baseline"} & set(d)
    a = np.load(tmp_path / "image_features.npy")
    assert a.dtype == np.float32 and a.shape == (2, 16, 896) and np.isfinite(a).all()


@pytest.mark.gpu
def test_full_run_carries_the_profiled_pass():
    r = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--res", "256", "--full", "--no-cpu-baseline")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["roofline"]["achieved"] > 0 and d["kernels"] and "power" in d
