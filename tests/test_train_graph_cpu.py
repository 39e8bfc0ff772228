"""CPU-side checks of the graph-captured train step (tactilesr_amd.train.graph.GraphedTrainStep): the host helper that
forms the Adam launch's per-step scalars, the new C-ABI entry points, and the refusal of a model that is not on a ROCm
device.  No compute calls."""
import ctypes
import math

import numpy as np
import pytest
import torch

import tactilesr_amd
from tactilesr_amd import _lib, optim


@pytest.mark.parametrize("lr,b1,b2,step", [
    (1e-3, 0.9, 0.999, 1), (1e-3, 0.9, 0.999, 2), (3.7e-4, 0.9, 0.999, 17), (1e-3, 0.9, 0.999, 5000),
    (2.5e-5, 0.8, 0.99, 1), (0.1, 0.5, 0.9999, 5000), (1e-3, 0.0, 0.0, 3),
])
def test_adam_hyper_is_the_double_formula_rounded_once(lr, b1, b2, step):
    out = (ctypes.c_float * 3)()
    assert _lib.load().tsr_adam_hyper(ctypes.c_float(lr), b1, b2, step, out) == 0
    want = np.array([lr, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)], dtype=np.float64).astype(np.float32)
    got = np.frombuffer(bytes(out), dtype=np.float32)
    assert got.tobytes() == want.tobytes(), (got, want)


def test_adam_hyper_rejects_step_zero():
    out = (ctypes.c_float * 3)()
    assert _lib.load().tsr_adam_hyper(ctypes.c_float(1e-3), 0.9, 0.999, 0, out) != 0


def test_library_exports_the_graph_step_entry_points_at_abi_24():
    lib = _lib.load()
    for name in ("tsr_adam_l2_multi_dev", "tsr_adam_hyper"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24


def test_graphed_train_step_refuses_a_cpu_model():
    from tactilesr_amd.train.graph import GraphedTrainStep
    from tactilesr_amd.train import tactileSR_train as TR
    torch.manual_seed(0)
    m = tactilesr_amd.TactileSR().train()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    with pytest.raises(_lib.TactileSRHipError, match="ROCm"):
        GraphedTrainStep(m, opt, TR.default_config())
