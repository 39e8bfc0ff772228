"""Host-side checks of the per-sample supervision weights: the yardstick of tests/_sample_weight_cases.py against torch's
own losses and autograd, how far plain fp32 is from the bar on every case, the scale's definition, the ABI, every refusal
(status 1 before any device call), the config key, the loader and eval_func on a stub.  No test here needs a device."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _sample_weight_cases as WC
import _ssim_cases as SC
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib
from tactilesr_amd.data.device_loader import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = _lib.TactileSRHipError
NAN, INF = WC.NAN, WC.INF


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("norm", list(WC.NORMS))
def test_restatement_is_torchs_per_sample_loss_weighted_by_hand(norm):
    y, t = (x.double() for x in WC.inputs(40, 40, 7))
    w = WC.weights_for(7, "fractional", seed=7)
    s = WC.scale_ref(w, norm)[0]
    for kind, param, fn in (("mse", None, lambda a, b: F.mse_loss(a, b)), ("l1", None, lambda a, b: F.l1_loss(a, b)),
                            ("huber", 0.25, lambda a, b: F.huber_loss(a, b, delta=0.25)),
                            ("huber", 1.0, lambda a, b: F.huber_loss(a, b, delta=1.0))):
        L, pix = WC.restatement(y, t, s, kind, param)
        want = [float(fn(y[b], t[b])) for b in range(7)]
        hand = sum(float(s[b]) * want[b] for b in range(7) if float(s[b]) != 0) / 7
        assert abs(float(L) - hand) <= 1e-12 * abs(hand), (kind, float(L), hand)
        for b in range(7):
            assert abs(float(pix[b]) - (want[b] if float(s[b]) != 0 else 0.0)) <= 1e-12 * want[b], (kind, b)
    if norm == "sum":                                               # the supervised term is the mean over the labeled weight
        L, _ = WC.restatement(y, t, s, "mse")
        wd = w.double()
        by_weight = sum(float(wd[b]) * float(F.mse_loss(y[b], t[b])) for b in range(7)) / float(wd.sum())
        assert abs(float(L) - by_weight) <= 1e-7 * by_weight         # s is an fp32 vector


@pytest.mark.parametrize("kind,param,fw,thr", WC.PARAMS, ids=[f"{k}-{p}-{w}" for k, p, w, _ in WC.PARAMS])
def test_closed_form_is_fp64_autograd(kind, param, fw, thr):
    for (H, W, B), pattern in (((5, 7, 7), "fractional"), ((40, 40, 7), "binary"), ((1, 1, 1), "ones"), ((3, 127, 7), "zeros")):
        y, t = WC.inputs(H, W, B)
        s = WC.scale_ref(WC.weights_for(B, pattern, seed=B), "sum")[0]
        pix, dy = WC.closed_form(y, t, s, kind, param, fw, thr)
        L, pix_a, dy_a = WC.autograd_grads(y, t, s, kind, param, fw, thr, torch.float64)
        scale = float(dy_a.abs().max())
        assert float((dy - dy_a).abs().max()) <= 1e-9 * scale, (kind, H, W, pattern)
        assert torch.equal(pix, pix_a)
        assert (dy[~WC.kept(s)] == 0).all() and (pix[~WC.kept(s)] == 0).all()


def test_restatement_never_reads_a_skipped_sample():
    y, t = WC.inputs(5, 7, 7)
    s = WC.scale_ref(WC.weights_for(7, "binary"), "sum")[0]
    yp, tp = WC.poisoned(y, t, s)
    assert torch.isnan(yp[1]).all() or torch.isinf(yp[1]).all()
    for kind, param, fw, thr in WC.PARAMS:
        a, b = WC.closed_form(y, t, s, kind, param, fw, thr), WC.closed_form(yp, tp, s, kind, param, fw, thr)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sref = SC.reference("w11_5x40x40", "clamped")
    s5 = torch.tensor([1.0, 0.0, 2.0, 0.0, 0.5])
    yp, tp = WC.poisoned(sref["y"].double(), sref["t"].double(), s5)
    args = (11, 1.5, sref["C1"], sref["C2"])
    clean = WC.restatement(sref["y"].double(), sref["t"].double(), s5, "mse", ssim_weight=0.1, ssim_args=args)[0]
    dirty = WC.restatement(yp, tp, s5, "mse", ssim_weight=0.1, ssim_args=args)[0]
    assert torch.equal(clean, dirty) and torch.isfinite(clean)


WORST32 = WC.Worst()


@pytest.mark.parametrize("H,W", list(WC.SHAPES), ids=[f"{h}x{w}" for h, w in WC.SHAPES])
@pytest.mark.parametrize("B", WC.BATCHES)
def test_fp32_restatement_stays_below_a_tenth_of_the_bar(H, W, B):
    """What gives the 1e-5 bar its factor of 10: on every case of the GPU tables the restatement in fp32 is within 1e-6."""
    for kind, param, fw, thr in WC.PARAMS:
        for pattern, norm in (("fractional", "sum"), ("ones", "sum"), ("fractional", "batch")):
            y, t = WC.inputs(H, W, B)
            s = WC.scale_ref(WC.weights_for(B, pattern, seed=B), norm)[0]
            ref = WC.build_reference(y, t, s, kind, param, fw, thr)
            fr = WC.fp32_fractions(ref)
            WORST32.take(fr)
            assert max(fr.values()) <= WC.FP32_BAR, (H, W, B, kind, param, fw, pattern, norm, fr)
    print(WORST32.line(f"fp32 restatement, up to {H}x{W} B={B}").replace(f"bar {WC.BAR:.0e}", f"bar {WC.FP32_BAR:.0e}"))


# ------------------------------------------------------------------------------------------------------------------ the scale
def test_scale_of_both_modes():
    for B in (1, 3, 32, 67, 600):
        for v in (1.0, 0.3, 7.0, 1e-30, 3e38 / 600):
            s, D, n = WC.scale_ref(torch.full((B,), v), "sum")
            assert (s == 1).all() and n == B, (B, v)                # uniform weights: exactly 1
            assert torch.equal(WC.scale_ref(torch.full((B,), v), "batch")[0], torch.full((B,), v))
        for norm in WC.NORMS:
            s, D, n = WC.scale_ref(torch.zeros(B), norm)
            assert (s == 0).all() and D == 0 and n == 0             # all unlabeled: everything skipped
    w = torch.tensor([1.0, -1.0, 3.0, NAN, 0.0, INF, 4.0, -INF, -0.0])
    for norm in WC.NORMS:
        s, D, n = WC.scale_ref(w, norm)
        assert D == 8.0 and n == 3                                  # the invalid ones are left out of D
        assert torch.isnan(s[[1, 3, 5, 7]]).all() and not torch.isnan(s[[0, 2, 4, 6, 8]]).any()
        assert float(s[4]) == 0 and float(s[8]) == 0 and not WC.kept(s)[[4, 8]].any() and WC.kept(s)[[1, 3, 5, 7]].all()
        want = w[[0, 2, 6]] * (9 / 8.0 if norm == "sum" else 1.0)
        assert torch.equal(s[[0, 2, 6]], want)
    s, D, n = WC.scale_ref(torch.tensor([NAN, -2.0]), "sum")
    assert D == 0 and n == 0 and torch.isnan(s).all()
    big = WC.weights_for(WC.INVALID_B, "invalid", seed=1)
    assert int((~WC.valid(big)).sum()) == 4 and big[WC.valid(big)].min() == 0
    sb = WC.scale_ref(big, "sum")[0]
    assert abs(float(sb[WC.valid(big)].double().sum()) - WC.INVALID_B) <= 1e-4      # the valid scales sum to B


def test_weighted_mean_reference():
    v = torch.tensor([1.0, NAN, 3.0, INF])
    assert WC.mean_ref(v, torch.tensor([1.0, 0.0, 2.0, 0.0])) == 7.0 / 4
    assert WC.mean_ref(v[[0, 2]], None) == 2.0
    assert WC.mean_ref(v, torch.zeros(4)) == 0.0
    import math
    assert math.isnan(WC.mean_ref(v, torch.tensor([1.0, NAN, 0.0, 0.0])))


# -------------------------------------------------------------------------------------------------------------------- the ABI
DECLS = {"tsr_sample_scale": 6, "tsr_pixel_loss_ps_fwd_bwd": 15, "tsr_pixel_loss_ps_fwd_bwd_wgs": 16, "tsr_ssim_fwd_bwd_ps": 15,
         "tsr_weighted_mean": 5}


def test_entry_points_are_declared_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    lib = _lib.load()
    for name, n_args in DECLS.items():
        decl = re.search(rf"^int\s+{name}\s*\(([^;]*)\)\s*;", header, re.M)
        assert decl, f"{name} is not declared in include/tactilesr_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n_args, name
        assert hasattr(lib, name)
    cap = re.search(r"^#define\s+TSR_PIXEL_LOSS_PS_MAX_WGS\s+(\d+)", header, re.M)
    assert cap and int(cap.group(1)) == Fh.PIXEL_LOSS_PS_MAX_WGS == WC.MAX_WGS
    assert Fh.SAMPLE_WEIGHT_NORMS == WC.NORMS
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24
    para = header[header.index("Per-sample supervision weights"):header.index("int tsr_sample_scale")]
    assert para.count("Refusals") >= 3 and "pix_b" in para and "mode 1" in para


@pytest.mark.parametrize("label,over", WC.PS_REFUSALS, ids=[r[0] for r in WC.PS_REFUSALS])
def test_pixel_ps_refusals_need_no_device(label, over):
    """Status 1 before any device call: the pointers are small fake addresses nothing may dereference."""
    for cap in (None, 8):
        a = dict(WC.PS_BASE, max_wgs=cap, **over) if "max_wgs" not in over else dict(WC.PS_BASE, **over)
        assert WC.call_ps(_lib.load(), a, **WC.fake_pointers(a, ("y", "t", "s", "pix", "dy", "dt"))) == 1, (label, cap)


@pytest.mark.parametrize("label,over", WC.SSIM_REFUSALS, ids=[r[0] for r in WC.SSIM_REFUSALS])
def test_ssim_ps_refusals_need_no_device(label, over):
    for s in (1, 0):
        a = dict(WC.SSIM_BASE, s=s, **over)
        assert WC.call_ssim_ps(_lib.load(), a, **WC.fake_pointers(a, ("y", "t", "s", "ssim", "dy"))) == 1, (label, s)


def test_scale_and_mean_refusals_need_no_device():
    lib = _lib.load()
    for label, over in WC.SCALE_REFUSALS:
        a = dict(WC.SCALE_BASE, **over)
        assert WC.call_scale(lib, a, **WC.fake_pointers(a, ("w", "s", "stats"))) == 1, label
    for label, over in WC.MEAN_REFUSALS:
        for s in (1, 0):
            a = dict(WC.MEAN_BASE, s=s, **over)
            assert WC.call_mean(lib, a, **WC.fake_pointers(a, ("v", "s", "out"))) == 1, (label, s)


def test_refusal_tables_cover_the_header():
    keys = {k for _, over in WC.PS_REFUSALS for k in over}
    assert keys >= {"y", "t", "B", "P", "pix", "kind", "param", "fg_weight", "fg_threshold", "accumulate", "dy", "dy_scale", "dt",
                    "max_wgs"}
    assert {k for _, over in WC.SCALE_REFUSALS for k in over} == {"w", "s", "stats", "B", "mode"}
    assert {k for _, over in WC.MEAN_REFUSALS for k in over} == {"v", "out", "B"}


# ------------------------------------------------------------------------------------------------------------- functional
def test_functional_refuses_on_the_host():
    y = torch.zeros(4, 1, 8, 8)
    w = torch.ones(4)
    for fn in (lambda: Fh.sample_scale(w), lambda: Fh.weighted_mean(w), lambda: Fh.pixel_loss_per_sample(y, y),
               lambda: Fh.sr_loss_fwd_bwd(y, y, sample_weight=w), lambda: Fh.sr_loss(y, y, 0.0, sample_weight=w)):
        with pytest.raises(ERR):                                    # CPU tensors: there is no fallback
            fn()
    for bad in ("mean", "", None, 0, "SUM "):
        with pytest.raises(ERR):
            Fh.sample_weight_norm_arg(bad)
    assert Fh.sample_weight_norm_arg("Sum") == "sum" and Fh.sample_weight_norm_arg("batch") == "batch"
    for fn in (Fh.sr_loss_fwd_bwd, Fh.sr_loss):
        sig = inspect.signature(fn).parameters
        assert sig["sample_weight"].default is None and sig["sample_weight_norm"].default == "sum"
    sig = inspect.signature(Fh.pixel_loss_per_sample).parameters
    assert list(sig)[:11] == ["y", "target", "kind", "param", "fg_weight", "fg_threshold", "scale", "dy", "dy_scale",
                              "accumulate", "want_dt"]
    assert list(inspect.signature(Fh.ssim).parameters) == ["a", "b", "data_range", "window", "sigma", "K1", "K2"]
    assert inspect.signature(Fh.sample_scale).parameters["norm"].default == "sum"


# ------------------------------------------------------------------------------------------------------------ the train glue
class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(2.0))

    def forward(self, x):
        return (self.w * x[:, :3].mean(dim=(1, 2, 3), keepdim=True)).expand(-1, 1, 40, 40).contiguous()


def test_sample_weight_config_and_the_batch_forms():
    conf = TR.default_config()
    assert "sample_weight_norm" not in conf and TR.sample_weight_config(conf) == "sum"
    assert TR.sample_weight_config(dict(conf, sample_weight_norm="batch")) == "batch"
    for bad in ("mean", None, 1, "labeled"):
        with pytest.raises(ERR):
            TR.sample_weight_config(dict(conf, sample_weight_norm=bad))
    LR, HR, g, w = torch.rand(4, 3, 4, 4), torch.rand(4, 1, 100, 100), torch.ones(4), torch.tensor([1.0, 0.0, 1.0, 0.5])
    assert TR._batch_weight((LR, HR), "cpu") is None and TR._batch_weight((LR, HR, g), "cpu") is None
    assert torch.equal(TR._batch_weight((LR, HR, None, w.double()), "cpu"), w)
    assert TR._batch_gamma((LR, HR, None, w), "cpu") is None and torch.equal(TR._batch_gamma((LR, HR, g, w), "cpu"), g)
    assert TR._batch_gamma((LR, HR), "cpu") is None and torch.equal(TR._batch_gamma((LR, HR, g), "cpu"), g)
    with pytest.raises(ERR, match="weight"):                        # the message names the new form
        TR._batch_gamma((LR, HR, g, w, w), "cpu")
    with pytest.raises(ERR):
        TR._batch_gamma((LR, HR, None), "cpu")                      # a 3-tuple's gamma is not optional
    ran = []

    class Spy(_Stub):
        def forward(self, x):
            ran.append(1)
            return super().forward(x)
    for c, batch in ((dict(conf, sample_weight_norm="mean"), (LR, HR, None, w)),
                     (conf, (LR, HR, None, torch.ones(3))), (conf, (LR, HR, None, torch.ones(4, 1))), (conf, (LR, HR, None, 1.0)),
                     (dict(conf, degradation_loss_weight=0.1, degradation_gamma=0.7), (LR, HR, torch.ones(3), w)),
                     (dict(conf, degradation_loss_weight=0.1), (LR, HR, None, w))):            # no gamma anywhere
        with pytest.raises(ERR):
            TR.train_cal_loss(Spy(), batch, c)
    assert not ran
    assert "SRLossSpec.from_config(self.config)" in inspect.getsource(GraphedTrainStep._key)   # the norm is in the key
    assert TR.SRLossSpec.from_config(dict(conf, sample_weight_norm="batch")) != TR.SRLossSpec.from_config(conf)


def test_eval_func_on_a_stub_with_and_without_weights():
    conf = TR.default_config()
    g = torch.Generator().manual_seed(71)
    n = 11
    LR, HR = torch.rand(n, 3, 4, 4, generator=g) * 8, torch.rand(n, 1, 100, 100, generator=g) * 100
    w = WC.weights_for(n, "fractional", seed=3)
    HRn = HR.clone()
    HRn[w == 0] = NAN                                               # an unlabeled sample's HR may hold anything
    names = ("mse_loss", "psnr_ssim", "prepare_target", "ssim", "sample_scale", "pixel_loss_per_sample", "weighted_mean")
    saved = [getattr(Fh, k) for k in names]
    Fh.mse_loss = lambda y, t: ((y - t) ** 2).mean()
    Fh.psnr_ssim = lambda y, t, m, reference_quirk=True: (-(y - t).abs().mean((1, 2, 3)), (y * t).mean((1, 2, 3)))
    Fh.ssim = lambda y, t, dr, win, sig: (y + t).mean((1, 2, 3))
    Fh.prepare_target = lambda h, s, f: h[:, :, 30:70, 30:70] / s
    calls = []

    def scale(wv, norm="sum"):
        calls.append(norm)
        s, D, cnt = WC.scale_ref(wv.float(), norm)
        return s, torch.tensor([D, cnt], dtype=torch.float32)
    Fh.sample_scale = scale
    Fh.pixel_loss_per_sample = lambda y, t, kind="mse", scale=None, **kw: (WC.per_sample(WC.masked(y, scale), WC.masked(t, scale), kind),
                                                                           None)
    Fh.weighted_mean = lambda v, s=None: torch.tensor([WC.mean_ref(v, s)])
    try:
        for bs in (4, 3):
            calls.clear()
            base = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, bs, device="cpu"), conf, windowed_ssim=True)
            assert not calls and len(base) == 4
            ones = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, bs, device="cpu", weight=torch.ones(n)), conf, windowed_ssim=True)
            assert calls and set(calls) == {"batch"}
            with torch.no_grad():
                out = _Stub()(LR)
            t = HR[:, :, 30:70, 30:70] / 10
            per = [((out - t) ** 2).mean((1, 2, 3)), (out * t).mean((1, 2, 3)), -(out - t).abs().mean((1, 2, 3)), (out + t).mean((1, 2, 3))]
            for got, m in zip(ones, per):                           # all weights 1: the mean over the SET, not over batches
                assert abs(got - float(m.double().mean())) <= 1e-6 * abs(float(m.double().mean()))
            got = TR.eval_func(_Stub(), DeviceSRLoader(LR, HRn, bs, device="cpu", weight=w), conf, windowed_ssim=True)
            three = TR.eval_func(_Stub(), DeviceSRLoader(LR, HRn, bs, device="cpu", weight=w), conf)
            assert tuple(three) == tuple(got[:3])
            for a, m in zip(got, per):
                want = float((w.double() * m.double()).sum() / w.double().sum())
                assert abs(a - want) <= 1e-6 * abs(want), (bs, a, want)
            none = TR.eval_func(_Stub(), DeviceSRLoader(LR, HRn, bs, device="cpu", weight=torch.zeros(n)), conf, windowed_ssim=True)
            assert len(none) == 4 and all(v != v for v in none)     # sum w = 0: NaN, not a division error
        mixed = [(LR[:4], HR[:4]), (LR[4:8], HR[4:8], None, torch.ones(4))]
        with pytest.raises(ERR):
            TR.eval_func(_Stub(), mixed, conf)
    finally:
        for k, v in zip(names, saved):
            setattr(Fh, k, v)


# ------------------------------------------------------------------------------------------------------------------ the loader
def _set(n=11):
    g = torch.Generator().manual_seed(5)
    return (torch.rand(n, 3, 4, 4, generator=g), torch.rand(n, 12, 12, generator=g), torch.arange(n, dtype=torch.float32) + 0.5,
            WC.weights_for(n, "fractional", seed=2) + torch.arange(n) * 4.0)       # distinct: a weight names its sample


@pytest.mark.parametrize("kw", [dict(), dict(shuffle=True, seed=3), dict(shuffle=True, seed=3, drop_last=True),
                                dict(shuffle=True, seed=4, world_size=2, rank=1)], ids=["plain", "shuffle", "drop_last", "rank"])
def test_loader_without_weight_is_the_loader_as_it_was(kw):
    LR, HR, gam, w = _set()
    a, b = DeviceSRLoader(LR, HR, 4, device="cpu", **kw), DeviceSRLoader(LR, HR, 4, device="cpu", weight=w, **kw)
    c, d = (DeviceSRLoader(LR, HR, 4, device="cpu", gamma=gam, **kw),
            DeviceSRLoader(LR, HR, 4, device="cpu", gamma=gam, weight=w, **kw))
    assert a.weight is None and c.weight is None
    for _ in range(2):                                              # two epochs: the generator state carries over
        n = 0
        for x, y, u, v in zip(a, b, c, d):
            assert len(x) == 2 and len(u) == 3 and len(y) == 4 and len(v) == 4 and a.last_index is None
            assert y[2] is None and torch.equal(v[2], u[2])
            for other in (y, u, v):
                assert torch.equal(x[0], other[0]) and torch.equal(x[1], other[1])
            assert y[3].dtype == torch.float32 and torch.equal(y[3], b.weight[b.last_index]) and torch.equal(v[3], y[3])
            assert torch.equal(y[0], b.LR[b.last_index])
            n += 1
        assert n == len(a) == len(b)
        for other in (b, c, d):
            assert torch.equal(a._gen.get_state(), other._gen.get_state())


@pytest.mark.parametrize("mode", ["random", "expand"])
def test_weight_follows_the_index_under_augmentation(mode):
    LR, HR, gam, w = _set()
    kw = dict(shuffle=True, seed=9, augment="dihedral", augment_mode=mode)
    a, b = DeviceSRLoader(LR, HR, 4, device="cpu", **kw), DeviceSRLoader(LR, HR, 4, device="cpu", weight=w, gamma=gam, **kw)
    seen = []
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(a.last_index, b.last_index)
        assert torch.equal(a.last_ops, b.last_ops) and torch.equal(y[3], w[b.last_index]) and torch.equal(y[2], gam[b.last_index])
        seen += b.last_index.tolist()
    assert torch.equal(a._gen.get_state(), b._gen.get_state())
    assert sorted(seen) == sorted(list(range(11)) * (8 if mode == "expand" else 1))


def test_loader_weight_arguments_and_entries():
    LR, HR, gam, w = _set()
    for bad in (w[:5], w.view(-1, 1)):
        with pytest.raises(ERR):
            DeviceSRLoader(LR, HR, 4, device="cpu", weight=bad)
    ld = DeviceSRLoader(LR, HR, 4, device="cpu", weight=w.double().numpy())
    assert ld.weight.dtype == torch.float32 and torch.equal(ld.weight, w)
    entries = [[{"LR": LR[i], "HR": HR[i], "alphaBeta": torch.tensor([1.0, 2.0, float(gam[i])])}] for i in range(11)]
    assert DeviceSRLoader.from_entries(entries, 4, device="cpu").weight is None
    ld = DeviceSRLoader.from_entries(entries, 4, device="cpu", with_weight=True)
    assert torch.equal(ld.weight, torch.ones(11)) and torch.equal(ld.HR, HR) and len(next(iter(ld))) == 4
    entries[2][0]["weight"] = 0.25                                  # an entry's own weight
    for i in (4, 9):                                                # recorded frames: no HR
        del entries[i][0]["HR"]
    ld = DeviceSRLoader.from_entries(entries, 4, device="cpu", with_weight=True, with_gamma=True)
    want = torch.ones(11)
    want[2], want[4], want[9] = 0.25, 0.0, 0.0
    assert torch.equal(ld.weight, want) and torch.equal(ld.gamma, gam)
    assert (ld.HR[[4, 9]] == 0).all() and ld.HR.shape == HR.shape and torch.equal(ld.HR[3], HR[3])
    lr, hr, g, ww = next(iter(ld))
    assert torch.equal(ww, want[:4]) and torch.equal(g, gam[:4])
    with pytest.raises(KeyError):                                   # without the flag an entry needs its HR, as before
        DeviceSRLoader.from_entries(entries, 4, device="cpu")
    for e in entries:
        e[0].pop("HR", None)
    with pytest.raises(ERR):                                        # nothing gives the HR shape
        DeviceSRLoader.from_entries(entries, 4, device="cpu", with_weight=True)
    sig = inspect.signature(DeviceSRLoader.from_file).parameters
    assert sig["with_weight"].default is False and inspect.signature(DeviceSRLoader.__init__).parameters["weight"].default is None


def test_from_file_with_weight(tmp_path):
    import numpy as np
    LR, HR, gam, w = _set(5)
    arr = np.empty((5, 1), dtype=object)                            # the on-disk layout of save_dataset
    for i in range(5):
        e = {"LR": LR[i].numpy(), "alphaBeta": np.array([1.0, 2.0, float(gam[i])])}
        if i != 3:
            e["HR"] = HR[i].numpy()
        if i == 1:
            e["weight"] = 2.5
        arr[i, 0] = e
    path = str(tmp_path / "set.npy")
    np.save(path, arr, allow_pickle=True)
    ld = DeviceSRLoader.from_file(path, 2, device="cpu", with_weight=True)
    assert torch.equal(ld.weight, torch.tensor([1.0, 2.5, 1.0, 0.0, 1.0])) and (ld.HR[3] == 0).all()
    assert torch.equal(ld.HR[4], HR[4])
