"""CPU side of the SSIM feature (tests/_ssim_cases.py): the yardstick is what it claims to be, the rule's second term is
capped on every case, the entry point is declared, every refusal is refused before any device call, the train glue
parses its optional keys, and the golden fixture agrees with the yardstick."""
import math
import os
import re

import pytest
import torch

import _ssim_cases as SC
from tactilesr_amd import _lib
from tactilesr_amd.train import tactileSR_train as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(c[0], law) for c in SC.WINDOW_CASES + SC.GLOBAL_CASES for law in SC.LAWS]


@pytest.mark.parametrize("win,sigma", [(11, 1.5), (5, 1.0), (0, 0.0)])
def test_restatement_equals_brute_force(win, sigma):
    y, t, _ = SC.make_pair(1, 12, 13, "signed", 1213)
    C1, C2 = SC.constants(1.0)
    got = float(SC.restatement(y.double(), t.double(), win, sigma, C1, C2))
    want = SC.brute_force(y[0, 0].double(), t[0, 0].double(), win, sigma, C1, C2)
    assert abs(got - want) <= 1e-12, (got, want)


@pytest.mark.parametrize("name", ["w11_3x13x29", "w7_3x13x29", "w3_2x5x7", "w11_1x11x11", "g_3x1x7", "g_4x40x40"])
@pytest.mark.parametrize("law", ["clamped", "signed", "pedestal", "dead"])
def test_closed_form_equals_autograd(name, law):
    ref = SC.reference(name, law)
    cf = SC.closed_form(ref["y"], ref["t"], ref["win"], ref["sigma"], ref["C1"], ref["C2"])
    err = (cf - ref["g64"]).abs().amax(dim=(1, 2, 3)) / ref["scale"]
    assert (err <= 1e-9).all(), err.tolist()


@pytest.mark.parametrize("name", [c[0] for c in SC.WINDOW_CASES + SC.GLOBAL_CASES])
def test_identical_images_give_one_and_no_gradient(name):
    for law in ("identical", "zeros"):
        ref = SC.reference(name, law)
        assert (ref["v64"] - 1).abs().max() <= 1e-12
        assert ((ref["g64"].abs().amax(dim=(1, 2, 3)) / ref["scale"]) <= 1e-9).all()


def test_second_term_is_capped_on_every_case():
    """The cap that keeps the rule from hiding a failure: 4 |fp32 restatement - fp64| <= 1e-3 of the scale."""
    worst_v = worst_g = 0.0
    for name, law in ALL:
        fv, fg = SC.second_term(SC.reference(name, law))
        assert float(fv.max()) <= SC.CAP and float(fg.max()) <= SC.CAP, (name, law, fv.tolist(), fg.tolist())
        worst_v, worst_g = max(worst_v, float(fv.max())), max(worst_g, float(fg.max()))
    for label, ref in [("walk", SC.walk_reference())]:
        fv, fg = SC.second_term(ref)
        assert (ref["scale"] > 0).all(), label
        assert float(fv.max()) <= SC.CAP and float(fg.max()) <= SC.CAP, (label, float(fv.max()), float(fg.max()))
        worst_v, worst_g = max(worst_v, float(fv.max())), max(worst_g, float(fg.max()))
    print(f"[ssim] second term, worst over {len(ALL)} cases: value {worst_v:.2e} gradient {worst_g:.2e} (cap {SC.CAP:.0e})")


def test_every_case_has_a_scale():
    for name, law in ALL:
        ref = SC.reference(name, law)
        assert (ref["scale"] > 0).all() and torch.isfinite(ref["g64"]).all() and torch.isfinite(ref["v64"]).all(), (name, law)


@pytest.mark.parametrize("H,W", SC.IMPULSE_SHAPES)
def test_impulse_images_have_a_gradient_of_their_own(H, W):
    ref = SC.impulse_reference(H, W)
    assert ref["y"].shape[0] == len(set(SC.impulse_positions(H, W, 11))) == 10
    assert (ref["scale"] > 0).all() and torch.isfinite(ref["g64"]).all()
    cf = SC.closed_form(ref["y"], ref["t"], 11, 1.5, ref["C1"], ref["C2"])
    assert ((cf - ref["g64"]).abs().amax(dim=(1, 2, 3)) / ref["scale"] <= 1e-7).all()


def test_entry_point_is_declared_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    decl = re.search(r"^int\s+tsr_ssim_fwd_bwd\s*\(([^;]*)\)\s*;", header, re.M)
    assert decl, "tsr_ssim_fwd_bwd is not declared in include/tactilesr_hip.h"
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["tsr_ssim_fwd_bwd"]) == 14
    lib = _lib.load()
    assert hasattr(lib, "tsr_ssim_fwd_bwd")
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24


@pytest.mark.parametrize("label,over", SC.REFUSALS, ids=[r[0] for r in SC.REFUSALS])
def test_refusals_need_no_device(label, over):
    """Status 1 before any device call: the pointers are small fake addresses nothing may dereference."""
    a = dict(SC.BASE_ARGS, **over)
    fake = lambda given: 64 if given else 0      # noqa: E731
    st = SC.call_raw(_lib.load(), a, y=fake(a["y"]), t=fake(a["t"]), ssim=fake(a["ssim"]), dy=fake(a["dy"]))
    assert st == 1, (label, st)


def test_refusal_table_covers_the_header():
    text = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    para = text[text.index("Differentiable SSIM"):text.index("int tsr_ssim_fwd_bwd")]
    assert "Refusals" in para
    keys = {k for _, over in SC.REFUSALS for k in over}
    assert keys >= {"y", "t", "ssim", "B", "H", "W", "win", "sigma", "C1", "C2", "accumulate", "dy_scale"}


def test_loss_config_keys():
    conf = TR.default_config()
    assert "ssim_loss_weight" not in conf                       # the fixture-pinned defaults stay as they are
    assert TR.ssim_loss_config(conf) == (0.0, 11, 1.5, 1.0)
    conf.update(ssim_loss_weight=0.1, ssim_window=7, ssim_sigma=1, ssim_data_range=20)
    got = TR.ssim_loss_config(conf)
    assert got == (0.1, 7, 1.0, 20.0) and [type(v) for v in got] == [float, int, float, float]


def test_cpu_tensors_are_refused():
    import tactilesr_amd.functional as Fh
    a = torch.zeros(1, 1, 12, 12)
    for fn in (Fh.ssim, Fh.ssim_loss, lambda x, y: Fh.sr_loss_fwd_bwd(x, y, 0.1)):
        with pytest.raises(_lib.TactileSRHipError):
            fn(a, a)


def test_golden_matches_the_restatement(golden):
    g = golden("ssim")
    y, t = torch.from_numpy(g["y"])[:, None], torch.from_numpy(g["t"])[:, None]
    assert y.shape == (2, 1, 24, 24) and y.dtype == torch.float32
    C1, C2 = SC.constants(1.0)
    v64, g64 = SC.values_and_grads(y, t, 0, 0.0, C1, C2, torch.float64)
    for key in ("calc_f64", "module_f64"):                      # calculationSSIM and SSIM()(.) are one formula
        assert (v64 - torch.from_numpy(g[key])).abs().max() <= 1e-12, key
    assert (g64[:, 0] - torch.from_numpy(g["grad_f64"])).abs().max() <= 1e-12 * max(1.0, float(g64.abs().max()))
    # the reference's own fp32 run is where the 1e-5 bar comes from: it must be a meaningful distance from fp64
    assert (torch.from_numpy(g["calc_f32"]) - v64).abs().max() <= 1e-3
    assert math.isfinite(float(g64.abs().max()))
