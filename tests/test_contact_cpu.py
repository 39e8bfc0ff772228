"""CPU checks of the contact readout: the yardstick of tests/_contact_cases.py against a brute-force double loop and the
closed forms, the preconditions of the GPU tables (the threshold margin, the share of images whose theta is checked), the
symbols and their refusals, the config keys, eval_func's default and the refusal of CPU tensors.  No GPU: refusals return
before any device call."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import _contact_cases as CC
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib
from tactilesr_amd.config import default as config_default
from tactilesr_amd.data.device_loader import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = _lib.TactileSRHipError
NAN, INF = CC.NAN, CC.INF
NAMES = ("tsr_contact_readout", "tsr_contact_readout_wgs")


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert (np.isnan(a) == np.isnan(b)).all(), (a, b)
    f = ~np.isnan(a)
    assert float(np.abs(a[f] - b[f]).max(initial=0.0)) <= tol, (a, b)


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (4, 4), (5, 7), (12, 20), (3, 31)])
def test_restatement_is_the_double_loop(H, W):
    for signed in (False, True):
        img = CC.blobs(5, H, W, seed=H + W, signed=signed)
        for mode, thr in CC.THRESHOLDS + [("abs", -0.125)]:
            for gain, span in ((1.0, (4.0, 4.0)), (10.0, (4.0, 6.0))):
                rec = CC.record(img, mode, thr, gain, span)
                for b in range(5):
                    want = CC.brute_force(img[b], mode, thr, gain, span)
                    th = [rec[b, 12], want[12]]
                    if not math.isnan(th[0]) and abs(abs(th[0]) - math.pi / 2) < 1e-9:      # the two ends of one axis
                        rec[b, 12], want[12] = abs(th[0]), abs(th[1])
                    got = rec[b].copy()
                    got[13:15], want[13:15] = got[13:15] ** 2, want[13:15] ** 2    # the eigenvalues: the root of a rounding
                    _close(got, want)                                               # residue next to 0 is not held to 1e-12


def test_restatement_pair_is_the_set_algebra():
    y, t = CC.shape_images(12, 20, 7)
    p, ry, rt = CC.pair(y, t, "abs", 0.3, 10.0, (4.0, 6.0))
    for b in range(7):
        my, mt = y[b] > np.float32(0.3), t[b] > np.float32(0.3)
        inter, uni = int((my & mt).sum()), int((my | mt).sum())
        assert p[b, 0] == inter and p[b, 1] == uni and abs(p[b, 2] - inter / uni) <= 1e-15
        assert abs(p[b, 3] - 2 * inter / (my.sum() + mt.sum())) <= 1e-15
        assert abs(p[b, 4] - math.hypot(ry[b, 7] - rt[b, 7], ry[b, 8] - rt[b, 8])) <= 1e-15
        assert abs(p[b, 5] - abs(ry[b, 2] - rt[b, 2]) / rt[b, 2]) <= 1e-15 and 0 <= p[b, 7] <= math.pi / 2
    _close(CC.pair(y, y, "range", 0.5)[0][:, 2:], np.array([[1, 1, 0, 0, 0, 0]] * 7), 0.0)
    empty = np.zeros((1, 8, 8), dtype=np.float32)
    one = CC.rectangle(8, 8, 2, 4, 2, 4)
    _close(CC.pair(empty, empty, "abs", 0.5)[0][0], [0, 0, 1, 1, NAN, NAN, 0, NAN])
    _close(CC.pair(empty, one, "abs", 0.5)[0][0, :6], [0, 4, 0, 0, NAN, 1])
    _close(CC.pair(one, empty, "abs", 0.5)[0][0, :6], [0, 4, 0, 0, NAN, NAN])
    bad = one.copy()
    bad[0, 0, 0] = NAN
    p, ry, rt = CC.pair(bad, one, "abs", 0.5)
    assert np.isnan(p).all() and np.isnan(ry).all() and not np.isnan(rt[:, :7]).any()


def test_restatement_closed_forms():
    for H, W in ((40, 40), (5, 7)):                                 # a one-pixel contact: its own centroid, no extent, no NaN
        for x, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
            r = CC.record(CC.impulses(H, W, [(x, c, 0.7001953125)]), "range", 0.5, 10.0, (4.0, 6.0))[0]
            assert r[0] == 1 and r[7] == (x + 0.5) * 4 / H - 0.5 and r[8] == (c + 0.5) * 6 / W - 0.5
            assert (r[9:15] == 0).all() and not np.isnan(r).any() and abs(r[2] - 7.001953125) < 1e-12
    r = CC.record(CC.rectangle(40, 40, 5, 17, 10, 16, 0.75), "abs", 0.0)[0]          # a constant rectangle
    _close(r[7:12], [11 * 0.1 - 0.5, 13 * 0.1 - 0.5, (144 - 1) / 12 * 0.01, (36 - 1) / 12 * 0.01, 0.0])
    assert abs(r[12]) < 1e-12 and r[0] == 72 and abs(r[1] - 0.72) < 1e-12
    r = CC.record(CC.rectangle(40, 40, 20, 24, 3, 30), "abs", 0.0)[0]
    assert abs(abs(r[12]) - math.pi / 2) < 1e-12
    for a, b, sp in (((10, 10), (20, 20), (4.0, 4.0)), ((10, 30), (30, 10), (4.0, 4.0)), ((3, 4), (13, 33), (4.0, 6.0))):
        r = CC.record(CC.impulses(40, 40, [a + (0.5,), b + (0.5,)]), "abs", 0.25, 1.0, sp)[0]       # two equal impulses
        du, dv = (b[0] - a[0]) * sp[0] / 40, (b[1] - a[1]) * sp[1] / 40
        d = abs(r[12] - math.atan2(dv, du))
        assert min(d, abs(math.pi - d)) < 1e-12 and abs(r[13] - math.hypot(du, dv) / 2) < 1e-12 and r[14] < 1e-7
    for n in (40, 100):                                             # a block over taxel (a, c): centroid (a, c), one pitch^2
        q = n // 4
        for a in range(4):
            for c in range(4):
                r = CC.record(CC.rectangle(n, n, a * q, (a + 1) * q, c * q, (c + 1) * q), "range", 0.5)[0]
                _close(r[[1, 7, 8]], [1.0, a, c])
    r = CC.record(CC.impulses(100, 100, [(12 + 25 * 2, 12 + 25 * 3, 1.0)]), "abs", 0.0)[0]
    assert r[5:9].tolist() == [2.0, 3.0, 2.0, 3.0]                 # the reference's mask centres are the taxel coordinates
    img = np.zeros((1, 8, 12), dtype=np.float32)                    # the comparison is strict
    img[0, 2, 3:7], img[0, 3, 3:6], img[0, 4, 4] = 0.5, 0.75, 1.0
    assert CC.record(img, "abs", 0.5)[0, 0] == 4 and CC.record(img, "range", 0.5)[0, 0] == 4
    assert CC.record(img, "range", 0.0)[0, 0] == 8 and CC.record(img, "abs", 7.0)[0, 0] == 0
    tie = np.zeros((1, 5, 7), dtype=np.float32)                     # the first maximum in row-major order
    tie[0, 4, 6] = tie[0, 2, 0] = tie[0, 4, 5] = 1.5
    assert CC.record(tie, "abs", 0.5)[0, 5:7].tolist() == [2.5 * 4 / 5 - 0.5, 0.5 * 4 / 7 - 0.5]


# ---------------------------------------------------------------------------------------------- what the GPU tables rely on
def _tables():
    for H, W in CC.SHAPES:
        for B in CC.BATCHES:
            yield (f"shapes {H}x{W} B={B}",) + CC.shape_images(H, W, B)
    yield "grid cap", CC.blobs(2100, 12, 20, seed=5), CC.blobs(2100, 12, 20, seed=6)
    yield "non-finite", CC.blobs(600, 12, 20, seed=21), CC.blobs(600, 12, 20, seed=22)
    yield "graph", CC.blobs(7, 40, 40, 91), CC.blobs(7, 40, 40, 92)


def test_no_pixel_sits_next_to_its_threshold():
    for name, y, t in _tables():
        for img in (y, t):
            assert (img * CC.Q == np.round(img * CC.Q)).all(), name   # multiples of 2^-10
            for mode, thr in CC.THRESHOLDS:
                assert CC.margin_ok(img, mode, thr), (name, mode, thr)
    signed = CC.blobs(7, 40, 40, seed=3, signed=True)
    assert (signed < 0).any() and CC.margin_ok(signed, "abs", -0.125) and CC.margin_ok(signed, "abs", 0.25)
    near = np.zeros((1, 4, 4), dtype=np.float32)                    # and the condition can fail
    near[0, 0, 0], near[0, 1, 1] = 1.0, np.float32(0.3) + np.float32(2e-7)
    assert not CC.margin_ok(near, "abs", 0.3) and CC.margin_ok(near, "abs", 0.5)
    near[0, 1, 1] = np.float32(0.3)                                 # a tie with an exactly representable tau is allowed
    assert CC.margin_ok(near, "abs", 0.3)


def test_ninety_percent_of_the_contacts_take_the_theta_check():
    """Per table and threshold: of the images with a contact, at least 90 % have theta held to 1e-5 (anisotropy >= 0.05)
    or to an exact 0 (a contact without extent, e.g. every 1x1 image)."""
    for name, y, t in _tables():
        for mode, thr in CC.THRESHOLDS:
            for img in (y, t):
                rec = CC.record(img, mode, thr)
                have = ~np.isnan(rec[:, 12])
                if not have.any():                                  # a 1x1 image under a range threshold: tau is the pixel
                    assert img.shape[1] * img.shape[2] == 1 and mode == "range", (name, mode, thr)
                    continue
                checked, aniso = CC.theta_checked(rec[have])
                assert checked.mean() >= 0.9, (name, mode, thr, float(checked.mean()))
                if img.shape[1] >= 12 and img.shape[2] >= 12:       # and on a real grid the blobs themselves are elongated
                    assert aniso.mean() >= 0.9, (name, mode, thr, float(aniso.mean()))


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_entry_points_are_declared_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24
    for name, n in zip(NAMES, (14, 15)):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
        assert decl, f"{name} is not declared in include/tactilesr_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n
        assert hasattr(lib, name)
    for macro, value in (("TSR_CONTACT_REC", CC.REC), ("TSR_CONTACT_PAIR", CC.PAIR), ("TSR_CONTACT_MAX_WGS", CC.MAX_WGS)):
        m = re.search(r"^#define\s+" + macro + r"\s+(\d+)", header, re.M)
        assert m and int(m.group(1)) == value, macro
    assert (Fh.CONTACT_REC, Fh.CONTACT_PAIR, Fh.CONTACT_MAX_WGS) == (CC.REC, CC.PAIR, CC.MAX_WGS) and Fh.CONTACT_MODES == CC.MODES
    para = header[header.index("Contact readout (csrc/contact_readout.hip)"):header.index("int tsr_contact_readout(")]
    for text in ("mn + threshold (mx - mn)", "the comparison is strict", "(x + 0.5) span_r / H - 0.5", "(c + 0.5) span_c / W - 0.5",
                 "0.5 atan2(2 muv, muu - mvv)", "first maximum in row-major order", "Non-finite input", "Refusals"):
        assert text in para, text
    src = open(os.path.join(REPO, "tactilesr_amd", "csrc", "contact_readout.hip")).read()
    assert "atomic" not in src.replace("atomics", "") and "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src
    assert "hipMemcpy" not in src and "getenv" not in src


def _fake(a):
    return CC.resolve_ptrs(a, dict(y=1 << 20, t=2 << 20, rec_y=3 << 20, rec_t=4 << 20, pair=5 << 20))


@pytest.mark.parametrize("label,over", CC.REFUSALS, ids=[r[0] for r in CC.REFUSALS])
def test_refusals_need_no_device(label, over):
    """Status 1 before any device call: the pointers are fake addresses nothing may dereference."""
    a = dict(CC.BASE_ARGS, **over)
    assert CC.call_raw(_lib.load(), a, **_fake(a)) == 1, label
    if "max_wgs" not in over:                                       # and the capped entry refuses the same
        assert CC.call_raw(_lib.load(), dict(a, max_wgs=4), **_fake(a)) == 1, label


def test_refusal_table_covers_the_header():
    text = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    para = text[text.index("Contact readout (csrc/contact_readout.hip)"):text.index("int tsr_contact_readout_wgs")]
    assert "Refusals" in para and "max_wgs < 1" in para
    keys = {k for _, over in CC.REFUSALS for k in over}
    assert keys >= {"y", "t", "rec_y", "rec_t", "pair", "B", "H", "W", "mode", "threshold", "gain", "span_r", "span_c", "max_wgs"}
    assert not {r[0] for r in CC.REFUSALS} & {r[0] for r in CC.ACCEPTED}
    for out in ("rec_y", "rec_t", "pair"):                          # every output against every input and every other output
        hit = {over[out].rstrip("+") for _, over in CC.REFUSALS if isinstance(over.get(out), str)}
        assert hit & {"y", "t"}, out
    assert any(over.get("rec_t") in ("rec_y", "rec_y+") for _, over in CC.REFUSALS)
    assert any(str(over.get("pair")).startswith("rec_") for _, over in CC.REFUSALS)


# ---------------------------------------------------------------------------------------------------- the functional layer
def test_cpu_tensors_and_bad_arguments_are_refused():
    y = torch.zeros(2, 1, 8, 8)
    for fn in (lambda: Fh.contact_readout(y), lambda: Fh.contact_metrics(y, y), lambda: Fh.contact_readout(y[:, 0]),
               lambda: Fh.sr_readout(torch.nn.Conv2d(1, 1, 1), y)):
        with pytest.raises(ERR, match="no CPU fallback"):
            fn()
    assert Fh.contact_readout_args() == (0.0, "abs", 1.0, (4.0, 4.0))
    assert Fh.contact_readout_args(0.5, "range", 10, (4, 6)) == (0.5, "range", 10.0, (4.0, 6.0))
    assert Fh.contact_readout_args(-3, "abs", -2.0, 5) == (-3.0, "abs", -2.0, (5.0, 5.0))
    for bad in (dict(mode="rel"), dict(mode=1), dict(threshold=NAN), dict(threshold=INF), dict(threshold="x"),
                dict(threshold=None), dict(mode="range", threshold=1.0), dict(mode="range", threshold=-0.01),
                dict(gain=NAN), dict(gain=-INF), dict(gain="x"), dict(span=(4.0, 0.0)), dict(span=(-4.0, 4.0)),
                dict(span=(4.0, NAN)), dict(span=(INF, 4.0)), dict(span=(1, 2, 3)), dict(span=(4,)), dict(span="wide"),
                dict(span=None), dict(span=0)):
        with pytest.raises(ERR):
            Fh.contact_readout_args(**bad)
    sig = inspect.signature(Fh.contact_readout).parameters
    assert list(sig) == ["y", "threshold", "mode", "gain", "span", "max_wgs"]
    assert [sig[k].default for k in list(sig)[1:]] == [0.0, "abs", 1.0, (4.0, 4.0), None]
    sig = inspect.signature(Fh.contact_metrics).parameters
    assert list(sig) == ["y", "t", "threshold", "mode", "gain", "span"]
    assert Fh.ContactReadout._fields == ("count", "area", "mass", "total", "peak", "peak_pos", "centroid", "moments", "angle",
                                         "major", "minor", "tau", "raw")
    assert Fh.ContactMetrics._fields == ("inter", "union", "iou", "dice", "centroid_dist", "mass_rel_err", "peak_dist",
                                         "angle_diff", "raw")


# ------------------------------------------------------------------------------------------------------------ the train glue
def test_contact_readout_config_keys():
    conf = TR.default_config()
    assert TR.contact_readout_config(conf) == (0.0, "abs", 10.0, (4.0, 4.0))
    got = TR.contact_readout_config(dict(conf, contact_threshold=0.5, contact_threshold_mode="range", contact_span=(4, 6),
                                         HR_scale_num=4))
    assert got == (0.5, "range", 4.0, (4.0, 6.0)) and [type(v) for v in got] == [float, str, float, tuple]
    assert TR.contact_readout_config(dict(conf, contact_span=5)) == (0.0, "abs", 10.0, (5.0, 5.0))
    assert TR.contact_readout_config({}) == (0.0, "abs", 1.0, (4.0, 4.0))            # every key is read with .get
    assert TR.pixel_loss_config(dict(conf, contact_threshold=0.5))[3] == 0.5         # the key the contact weight reads
    for bad in (dict(contact_threshold=NAN), dict(contact_threshold=INF), dict(contact_threshold="x"),
                dict(contact_threshold_mode="rel"), dict(contact_threshold_mode=None),
                dict(contact_threshold_mode="range", contact_threshold=1.0),
                dict(contact_threshold_mode="range", contact_threshold=-0.5), dict(contact_span=(4, 0)),
                dict(contact_span=(4, 4, 4)), dict(contact_span=-1), dict(contact_span="x"), dict(HR_scale_num=NAN),
                dict(HR_scale_num="x")):
        with pytest.raises(ERR):
            TR.contact_readout_config({**conf, **bad})


def test_default_config_dicts_are_unchanged():
    import json
    assert set(TR.default_config()) == {"HR_scale_num", "axisCnt", "lr", "scale_factor", "seqsCnt", "sensorMaxVaule_factor",
                                        "test_batch_size", "train_batch_size", "weight_decay"}
    ref = json.load(open(os.path.join(REPO, "tests", "golden", "config_default.json")))
    for name, rd in ref.items():                                    # the key sets the golden file pins
        assert set(getattr(config_default, name)) == set(rd), name
        assert not {"contact_threshold", "contact_threshold_mode", "contact_span"} & set(rd), name


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(2.0))

    def forward(self, x):
        return (self.w * x[:, :3].mean(dim=(1, 2, 3), keepdim=True)).expand(-1, 1, 40, 40).contiguous()


def test_eval_func_default_is_unchanged_on_a_stub():
    sig = inspect.signature(TR.eval_func).parameters
    assert sig["contact"].default is False and sig["degradation"].default is False
    assert list(sig)[:8] == ["model", "test_loader", "config", "windowed_ssim", "self_ensemble", "ema", "taxel_noise",
                             "noise_seed"]
    conf = TR.default_config()
    g = torch.Generator().manual_seed(71)
    LR, HR = torch.rand(12, 3, 4, 4, generator=g) * 8, torch.rand(12, 1, 100, 100, generator=g) * 100
    saved = Fh.mse_loss, Fh.psnr_ssim, Fh.prepare_target, Fh.contact_metrics
    Fh.mse_loss = lambda y, t: ((y - t) ** 2).mean()
    Fh.psnr_ssim = lambda y, t, m, reference_quirk=True: (-(y - t).abs().mean((1, 2, 3)), (y * t).mean((1, 2, 3)))
    Fh.prepare_target = lambda h, s, f: h[:, :, 30:70, 30:70] / s
    calls = []

    def fake(y, t, threshold=0.0, mode="abs", gain=1.0, span=(4.0, 4.0)):         # the yardstick in place of the launch
        calls.append((threshold, mode, gain, span))
        p, ry, rt = CC.pair(y[:, 0].numpy(), t[:, 0].numpy(), mode, threshold, gain, span)
        return (Fh._contact_metrics_of(torch.from_numpy(p).float()), None, None)
    Fh.contact_metrics = fake
    try:
        base = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), conf)
        off = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), conf, contact=False)
        assert base == off and len(base) == 3 and not calls
        want0 = (float(sum(((_Stub()(LR[i:i + 4]).detach() - HR[i:i + 4, :, 30:70, 30:70] / 10) ** 2).mean() for i in (0, 4, 8))) / 3)
        assert abs(base[0] - want0) <= 1e-6 * want0                 # today's tuple: the mean of the batch losses
        c = dict(conf, contact_threshold=0.5, contact_threshold_mode="range", contact_span=(4, 6))
        on = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), c, contact=True)
        assert on[:3] == base and len(on) == 6 and calls == [(0.5, "range", 10.0, (4.0, 6.0))] * 3
        out = _Stub()(LR).detach()
        p = CC.pair(out[:, 0].numpy(), (HR[:, 0, 30:70, 30:70] / 10).numpy(), "range", 0.5, 10.0, (4.0, 6.0))[0]
        for got, col in zip(on[3:], (2, 4, 5)):                     # sample means over the set, NaN samples left out
            v = p[:, col].astype(np.float32).astype(np.float64)
            want = v[~np.isnan(v)].mean() if (~np.isnan(v)).any() else NAN
            assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)
        with pytest.raises(ERR):                                    # a bad key raises before the loop
            TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), dict(conf, contact_threshold_mode="rel"), contact=True)
    finally:
        Fh.mse_loss, Fh.psnr_ssim, Fh.prepare_target, Fh.contact_metrics = saved


def test_contact_sums_are_whole_set_weighted_means_without_the_nans():
    s = TR._ContactSums()
    assert all(math.isnan(v) for v in s.means())
    a = torch.zeros(3, 8)
    a[:, 2], a[:, 4], a[:, 5] = torch.tensor([1.0, 0.5, 0.0]), torch.tensor([NAN, 2.0, 4.0]), torch.tensor([NAN, NAN, NAN])
    b = torch.zeros(2, 8)
    b[:, 2], b[:, 4], b[:, 5] = torch.tensor([0.25, 0.75]), torch.tensor([6.0, NAN]), torch.tensor([NAN, NAN])
    s.add(a)
    s.add(b)
    got = s.means()
    assert got[0] == 2.5 / 5 and got[1] == 12.0 / 3 and math.isnan(got[2])            # not the mean of the batch means
    w = TR._ContactSums()
    w.add(a, torch.tensor([2.0, 0.0, 1.0]))
    w.add(b, torch.tensor([1.0, 4.0]))
    got = w.means()
    assert got[0] == (2.0 * 1.0 + 0.25 + 4 * 0.75) / 8.0 and got[1] == (4.0 + 6.0) / 2.0 and math.isnan(got[2])
