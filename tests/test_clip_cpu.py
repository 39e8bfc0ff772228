"""CPU-side checks of gradient-norm clipping (the reference ``Trainer(clip_grad_norm=...)``, cpu/trainer.py:354-356):
the three C-ABI entry points are declared, bound and exported at an unchanged ABI, the trainer glue and the graphed step
take the option, and the graphed step still refuses a CPU model.  No compute calls."""
import inspect
import os

import pytest
import torch

import tactilesr_amd
from tactilesr_amd import _lib, optim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsr_grad_norm_multi", "tsr_adam_l2_multi_clip", "tsr_adam_l2_multi_dev_clip")


def test_header_declares_the_clip_entry_points():
    with open(os.path.join(REPO, "include", "tactilesr_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert f"int {name}(" in header, name
    assert "chunk.grad" in header          # the clipping Adam forms write the clipped gradient back


def test_library_exports_the_clip_entry_points_at_abi_24():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["tsr_adam_l2_multi_clip"] == _lib.SIGNATURES["tsr_adam_l2_multi"][:-1] + [_lib._P, _lib._P]
    assert (_lib.SIGNATURES["tsr_adam_l2_multi_dev_clip"]
            == _lib.SIGNATURES["tsr_adam_l2_multi_dev"][:-1] + [_lib._P, _lib._P])
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24


def test_clip_entry_points_reject_null_arguments():
    """Argument checks run on the host before any launch: NULL tables, buffers and coefficient pointers are refused."""
    import ctypes
    lib = _lib.load()
    fake = ctypes.c_void_p(16)           # never dereferenced: every call below fails its argument check first
    null = ctypes.c_void_p(0)
    assert lib.tsr_grad_norm_multi(null, 1, ctypes.c_float(1.0), fake, fake, null) != 0
    assert lib.tsr_grad_norm_multi(fake, 0, ctypes.c_float(1.0), fake, fake, null) != 0
    assert lib.tsr_grad_norm_multi(fake, 1, ctypes.c_float(1.0), null, fake, null) != 0
    assert lib.tsr_grad_norm_multi(fake, 1, ctypes.c_float(1.0), fake, null, null) != 0
    f = ctypes.c_float
    assert lib.tsr_adam_l2_multi_clip(fake, 1, f(1e-3), 0.9, 0.999, f(1e-8), f(0.0), 1, null, null) != 0
    assert lib.tsr_adam_l2_multi_clip(fake, 1, f(1e-3), 0.9, 0.999, f(1e-8), f(0.0), 0, fake, null) != 0
    assert lib.tsr_adam_l2_multi_dev_clip(fake, 1, fake, 0.9, 0.999, f(1e-8), f(0.0), null, null) != 0
    assert lib.tsr_adam_l2_multi_dev_clip(fake, 1, null, 0.9, 0.999, f(1e-8), f(0.0), fake, null) != 0


def test_trainer_glue_and_graphed_step_take_clip_grad_norm():
    from tactilesr_amd.train import tactileSR_train as TR
    from tactilesr_amd.train.graph import GraphedTrainStep
    p = inspect.signature(TR.train_one_iter).parameters["clip_grad_norm"]
    assert p.default == 0.0
    p = inspect.signature(GraphedTrainStep).parameters["clip_grad_norm"]
    assert p.default == 0.0
    assert "max_norm" in inspect.signature(optim.Adam.step_clipped).parameters
    assert "clip" in inspect.signature(optim.Adam._captured_step).parameters


def test_fused_clip_condition_is_parameter_identity():
    from tactilesr_amd.train import tactileSR_train as TR
    m = torch.nn.Linear(3, 2)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    assert TR.fused_clip_applies(m, optim.Adam(m.parameters()))
    assert not TR.fused_clip_applies(m, torch.optim.Adam(m.parameters()))
    assert not TR.fused_clip_applies(m, optim.Adam([m.weight]))            # holds only part of the model
    stale = torch.nn.Parameter(torch.zeros(4))                              # a discarded module's parameter
    assert TR.fused_clip_applies(m, optim.Adam(list(m.parameters()) + [stale]))
    stale.grad = torch.zeros(4)
    assert not TR.fused_clip_applies(m, optim.Adam(list(m.parameters()) + [stale]))


def test_graphed_train_step_with_clipping_refuses_a_cpu_model():
    from tactilesr_amd.train.graph import GraphedTrainStep
    from tactilesr_amd.train import tactileSR_train as TR
    torch.manual_seed(0)
    m = tactilesr_amd.TactileSR().train()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    with pytest.raises(_lib.TactileSRHipError, match="ROCm"):
        GraphedTrainStep(m, opt, TR.default_config(), clip_grad_norm=1.0)
