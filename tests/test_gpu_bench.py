"""A plain `python bench.py` run as a fresh process: one compact result line whose `steps` / `ms_per_step` follow the
arguments, none of what `--full` adds, and `--dump-outputs` files holding what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0], r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_infer_run_is_lean_and_dumps_the_last_step(tmp_path):
    runs = {}
    for steps in (1, 3):
        d = _bench("--gpus", "1", "--batch", "64", "--steps", str(steps), "--warmup", "1",
                   "--dump-outputs", str(tmp_path / str(steps)))
        assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["unit"] == "samples/s" and d["higher_is_better"] is True and isinstance(d["dtype"], str)
        assert d["ms_per_step"] > 0 and abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) <= 1e-2 * d["value"]
        for k in ("legs", "roofline", "whole_step", "f32_mfma_path", "cpu_baseline", "parity"):
            assert k not in d, k
        assert len(json.dumps(d)) < 4096                             # a compact line a driver can read back
        assert os.listdir(tmp_path / str(steps)) == ["output.npy"]
        runs[steps] = np.load(tmp_path / str(steps) / "output.npy")
    y1, y3 = runs[1], runs[3]
    assert y1.dtype == np.float32 and y1.shape == (64, 1, 40, 40) and np.isfinite(y1).all() and np.abs(y1).max() > 0
    # same seeded model and inputs, eval forward: the last step of either run computes the same image
    assert np.abs(y3 - y1).max() <= 1e-6 * np.abs(y1).max()


def test_plain_train_run_dumps_loss_and_updated_state(tmp_path):
    d = _bench("--mode", "train", "--batch", "16", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and "roofline" not in d and "cpu_baseline" not in d
    names = set(os.listdir(tmp_path))
    assert "total_loss.npy" in names and "state.output_layer.2.weight.npy" in names
    assert float(np.load(tmp_path / "total_loss.npy")) == pytest.approx(d["loss"], rel=1e-6)
    total = sum(os.path.getsize(tmp_path / n) for n in names)
    assert total < 64_000_000
    for n in names:
        a = np.load(tmp_path / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n


def test_plain_tpsf_run_dumps_loss_and_updated_state(tmp_path):
    d = _bench("--mode", "tpsf", "--batch", "256", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and "forward_only" not in d and "cpu_baseline" not in d
    names = set(os.listdir(tmp_path))
    assert "loss.npy" in names and "state.MLP_layer.7.weight.npy" in names
    assert float(np.load(tmp_path / "loss.npy")) == pytest.approx(d["loss"], rel=1e-6)
