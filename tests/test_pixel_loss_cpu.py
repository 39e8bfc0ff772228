"""CPU side of the pixel-loss feature (tests/_pixel_loss_cases.py): the yardstick is what it claims to be, plain fp32
stays a factor of 10 inside the bar on every case, the entry point is declared and bound at ABI 24, every refusal is
refused before any device call, and the train glue parses its optional keys."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _pixel_loss_cases as PC
from tactilesr_amd import _lib
from tactilesr_amd.train import tactileSR_train as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = list(PC.SIZES) + ["align"]


@pytest.mark.parametrize("name", ["n257", "b2_40"])
def test_restatement_equals_torch(name):
    y, t = (x.double() for x in PC.inputs(name))
    assert abs(float(PC.restatement(y, t, "mse")) - float(F.mse_loss(y, t))) <= 1e-12
    assert abs(float(PC.restatement(y, t, "l1")) - float(F.l1_loss(y, t))) <= 1e-12
    for delta in PC.DELTAS:
        assert abs(float(PC.restatement(y, t, "huber", delta)) - float(F.huber_loss(y, t, delta=delta))) <= 1e-12
    for eps in (1e-3, 0.1):
        hand = sum(((a - b) ** 2 + eps ** 2) ** 0.5 for a, b in zip(y.flatten().tolist(), t.flatten().tolist())) / y.numel()
        assert abs(float(PC.restatement(y, t, "charbonnier", eps)) - hand) <= 1e-12


@pytest.mark.parametrize("name", ["n3", "k3r3", "b2_40"])
@pytest.mark.parametrize("kind,param,fg_weight,fg_threshold", PC.PARAMS)
def test_closed_form_equals_autograd(name, kind, param, fg_weight, fg_threshold):
    ref = PC.reference(name, kind, param, fg_weight, fg_threshold)
    cf = PC.closed_form(ref["y"], ref["t"], kind, param, fg_weight, fg_threshold)
    assert float((cf - ref["g64"]).abs().max()) <= 1e-12
    assert torch.equal(ref["gt64"], -ref["g64"])                    # the target gradient: the weight is not differentiated


@pytest.mark.parametrize("kind,param", PC.KINDS)
def test_weight_zero_is_the_unweighted_form(kind, param):
    y, t = (x.double() for x in PC.inputs("b2_40"))
    plain = PC.restatement(y, t, kind, param)
    for thr in (0.0, 0.5, -1.0):
        assert torch.equal(PC.restatement(y, t, kind, param, 0.0, thr), plain)
    assert float(PC.restatement(y, t, kind, param, 4.0, 0.0)) > float(plain)      # and a weight is seen


def test_contact_weight_counts_the_right_pixels():
    y, t = PC.inputs("b2_40")
    for thr in (0.0, 0.5):
        w = PC.weights(t, 4.0, thr, torch.float64)
        assert torch.equal(w == 5, t > thr) and torch.equal(w == 1, t <= thr)
    assert 0.05 < float((t > 0).float().mean()) < 0.4 and float((t > 0.5).float().mean()) < float((t > 0).float().mean())
    nan_t = t.clone()
    nan_t[0, 0, 0, 0] = float("nan")
    assert PC.weights(nan_t, 4.0, 0.0, torch.float64)[0, 0, 0, 0] == 1      # a NaN target compares false


@pytest.mark.parametrize("name", TABLE + [PC.BIG])
def test_every_table_holds_ties_and_delta_pixels(name):
    y, t = PC.inputs(name)
    assert (t >= 0).all() and (y >= 0).all()
    d = (y.double() - t.double()).flatten()
    n = d.numel()
    if n >= 4:
        assert int((d == 0).sum()) >= n // 7
        assert ((y.flatten() == t.flatten())[3::7]).all()
    if n >= 16 and name != PC.BIG:                                  # the big case scales its strides: delta moves with them
        for delta in PC.DELTAS:
            assert (d == delta).any() and (d == -delta).any(), (name, delta)
    if n >= 1000:
        assert 0.05 < float((t > 0).float().mean()) < 0.4
    if name == PC.BIG:
        assert n == PC.BIG_N and n > 3 * PC.STRIDE and (n - 3 * PC.STRIDE) % 4 == 3


@pytest.mark.parametrize("name", TABLE)
def test_fp32_restatement_stays_a_factor_of_ten_inside_the_bar(name):
    """The condition that lets the bar do without the rule's second term."""
    worst = (0.0, 0.0)
    for kind, param, w, thr in PC.PARAMS:
        ref = PC.reference(name, kind, param, w, thr)
        fl, fg = PC.fp32_fractions(ref)
        assert fl <= PC.FP32_BAR and fg <= PC.FP32_BAR, (name, kind, param, w, thr, fl, fg)
        worst = (max(worst[0], fl), max(worst[1], fg))
    print(f"[pixel loss] fp32 restatement vs fp64, {name}: loss {worst[0]:.2e} gradient {worst[1]:.2e} of the scale")


@pytest.mark.parametrize("kind,param,fg_weight,fg_threshold", [("mse", None, 0.0, 0.0), ("huber", 0.25, 4.0, 0.5)])
def test_fp32_restatement_on_the_big_case(kind, param, fg_weight, fg_threshold):
    fl, fg = PC.fp32_fractions(PC.reference(PC.BIG, kind, param, fg_weight, fg_threshold))
    assert fl <= PC.FP32_BAR and fg <= PC.FP32_BAR, (fl, fg)


def test_entry_point_is_declared_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    decl = re.search(r"^int\s+tsr_pixel_loss_fwd_bwd\s*\(([^;]*)\)\s*;", header, re.M)
    assert decl, "tsr_pixel_loss_fwd_bwd is not declared in include/tactilesr_hip.h"
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["tsr_pixel_loss_fwd_bwd"]) == 14
    work = re.search(r"^#define\s+TSR_PIXEL_LOSS_WORK\s+(\d+)", header, re.M)
    import tactilesr_amd.functional as Fh
    assert work and int(work.group(1)) == Fh.PIXEL_LOSS_WORK == PC.WORK == 2048
    lib = _lib.load()
    assert hasattr(lib, "tsr_pixel_loss_fwd_bwd")
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24


@pytest.mark.parametrize("label,over", PC.REFUSALS, ids=[r[0] for r in PC.REFUSALS])
def test_refusals_need_no_device(label, over):
    """Status 1 before any device call: the pointers are small fake addresses nothing may dereference."""
    a = dict(PC.BASE_ARGS, **over)
    addr = dict(y=64, t=128, loss=192, dy=256, dt=320, work=384)
    ptrs = {k: (addr["dy"] if a[k] == "dy" else (addr[k] if a[k] else 0)) for k in addr}
    assert PC.call_raw(_lib.load(), a, **ptrs) == 1, label


def test_refusal_table_covers_the_header():
    text = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    para = text[text.index("Pixel losses of the train step"):text.index("int tsr_pixel_loss_fwd_bwd")]
    assert "Refusals" in para
    keys = {k for _, over in PC.REFUSALS for k in over}
    assert keys >= {"y", "t", "loss", "work", "n", "kind", "param", "fg_weight", "fg_threshold", "accumulate", "dy", "dy_scale",
                    "dt"}


def test_pixel_loss_config_keys():
    conf = TR.default_config()
    assert not {"pixel_loss", "pixel_loss_param", "contact_loss_weight", "contact_threshold"} & set(conf)
    assert TR.pixel_loss_config(conf) == ("mse", None, 0.0, 0.0) and TR.pixel_is_plain_mse(TR.pixel_loss_config(conf))
    assert TR.pixel_loss_config(dict(conf, pixel_loss="charbonnier")) == ("charbonnier", 1e-3, 0.0, 0.0)
    assert TR.pixel_loss_config(dict(conf, pixel_loss="huber")) == ("huber", 1.0, 0.0, 0.0)
    got = TR.pixel_loss_config(dict(conf, pixel_loss="Huber", pixel_loss_param=2, contact_loss_weight=4, contact_threshold=1))
    assert got == ("huber", 2.0, 4.0, 1.0) and [type(v) for v in got] == [str, float, float, float]
    assert TR.pixel_loss_config(dict(conf, pixel_loss="l1", pixel_loss_param=3)) == ("l1", None, 0.0, 0.0)     # not read
    assert not TR.pixel_is_plain_mse(TR.pixel_loss_config(dict(conf, contact_loss_weight=4)))
    assert not TR.pixel_is_plain_mse(TR.pixel_loss_config(dict(conf, pixel_loss="l1")))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(pixel_loss="l2"), dict(pixel_loss=None), dict(pixel_loss="huber", pixel_loss_param=0),
                dict(pixel_loss="huber", pixel_loss_param=nan), dict(pixel_loss="charbonnier", pixel_loss_param=-1e-3),
                dict(pixel_loss="charbonnier", pixel_loss_param=inf), dict(pixel_loss="charbonnier", pixel_loss_param="x"),
                dict(contact_loss_weight=-1), dict(contact_loss_weight=nan), dict(contact_loss_weight=inf),
                dict(contact_threshold=nan)):
        with pytest.raises(_lib.TactileSRHipError):
            TR.pixel_loss_config(dict(conf, **bad))


def test_cpu_tensors_are_refused():
    import tactilesr_amd.functional as Fh
    a = torch.zeros(1, 1, 12, 12)
    for fn in (Fh.pixel_loss, Fh.pixel_loss_fwd_bwd, lambda x, y: Fh.sr_loss_fwd_bwd(x, y, 0.0, pixel_kind="l1"),
               lambda x, y: Fh.sr_loss(x, y, 0.1, pixel_kind="l1")):
        with pytest.raises(_lib.TactileSRHipError):
            fn(a, a)
