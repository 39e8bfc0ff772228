"""bench.py's `--dump-outputs` writer on host tensors: dtypes, exact values under the size cap, and the seeded sample
past it (same positions from run to run, the whole dump within the cap)."""
import importlib.util
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("tsr_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float32_and_float64_exactly(tmp_path):
    b = _bench()
    g = torch.Generator().manual_seed(0)
    out = torch.rand(4, 1, 40, 40, generator=g, requires_grad=True) * 3
    loss = torch.tensor(1.25, dtype=torch.float64)
    half = torch.rand(8, generator=g).to(torch.bfloat16)
    b.dump_outputs(str(tmp_path), {"output": out, "loss": loss, "state.h": half,
                                   "state.n": torch.tensor(7, dtype=torch.int64)})
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "output.npy", "state.h.npy", "state.n.npy"]
    a = np.load(tmp_path / "output.npy")
    assert a.dtype == np.float32 and a.shape == (4, 1, 40, 40)
    assert np.array_equal(a, out.detach().numpy())
    assert np.load(tmp_path / "loss.npy").dtype == np.float64 and float(np.load(tmp_path / "loss.npy")) == 1.25
    h = np.load(tmp_path / "state.h.npy")
    assert h.dtype == np.float32 and np.array_equal(h, half.float().numpy())
    n = np.load(tmp_path / "state.n.npy")
    assert n.dtype == np.float64 and float(n) == 7.0


def test_dump_outputs_samples_past_the_cap_at_fixed_positions(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BYTES", 40_000)
    x = torch.arange(30_000, dtype=torch.float32)               # 120 kB
    w = torch.arange(5_000, dtype=torch.float64) * 0.5           # 40 kB
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"output": x, "w": w})
    xa, wa = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "a" / "w.npy")
    assert xa.nbytes + wa.nbytes <= 40_000
    assert xa.size == 30_000 // 4 and wa.size == 5_000 // 4        # the same fraction of every array
    assert np.all(np.diff(xa) > 0) and np.all(np.isin(xa, x.numpy()))   # sorted positions, values taken as they were
    assert wa.dtype == np.float64 and np.all(np.isin(wa, w.numpy()))
    assert np.array_equal(xa, np.load(tmp_path / "b" / "output.npy"))
    assert np.array_equal(wa, np.load(tmp_path / "b" / "w.npy"))
