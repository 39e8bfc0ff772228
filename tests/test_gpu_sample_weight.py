"""GPU checks of the per-sample supervision weights (tsr_sample_scale, tsr_pixel_loss_ps_fwd_bwd[_wgs], tsr_ssim_fwd_bwd_ps,
tsr_weighted_mean; functional.sample_scale / pixel_loss_per_sample / weighted_mean / sr_loss_fwd_bwd; the 4-tuple batch of
train_cal_loss, GraphedTrainStep, eval_func and DeviceSRLoader) against the fp64 restatement and the bar of
tests/_sample_weight_cases.py.  Every output buffer is prefilled with NaN between NaN guard bands, and every raw launch
runs twice and must give the same bits."""
import copy
import math

import pytest
import torch

import _degrade_cases as DC
import _gradcheck
import _sample_weight_cases as WC
import _ssim_cases as SC
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib, optim
from tactilesr_amd.data.device_loader import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

pytestmark = pytest.mark.gpu

NAN, INF = WC.NAN, WC.INF
bits = WC.bits
WORST = {k: WC.Worst() for k in ("shapes", "walk", "dy", "ssim")}


def _same(a, b, label=""):
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), (label, k)


# ------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("H,W", list(WC.SHAPES), ids=[f"{h}x{w}" for h, w in WC.SHAPES])
@pytest.mark.parametrize("B", WC.BATCHES)
def test_shapes_kinds_and_fractional_weights(H, W, B):
    y, t = WC.inputs(H, W, B)
    for kind, param, fw, thr in WC.PARAMS:
        ref = WC.reference(H, W, B, "fractional", "sum", kind, param, fw, thr)
        got = WC.launch_ps(y, t, ref["s"], kind, param, fw, thr)
        WC.check(ref, got["pix"], got["dy"], got["dt"], WORST["shapes"], label=(H, W, B, kind, param, fw))
    print(WORST["shapes"].line(f"shapes, up to {H}x{W} B={B}"))


def test_grid_caps_do_not_change_a_bit():
    """2100 distinct images: more than the default cap; caps of 1 and 3 walk them at another stride."""
    B, H, W = WC.WALK
    y, t = WC.inputs(H, W, B)
    for kind, param, fw, thr in (("mse", None, 0.0, 0.0), ("huber", 0.25, 4.0, 0.5)):
        ref = WC.reference(H, W, B, "fractional", "sum", kind, param, fw, thr)
        base = WC.launch_ps(y, t, ref["s"], kind, param, fw, thr)
        WC.check(ref, base["pix"], base["dy"], base["dt"], WORST["walk"], label=("walk", kind))
        for cap in (1, 3, WC.MAX_WGS, 5000):
            _same(base, WC.launch_ps(y, t, ref["s"], kind, param, fw, thr, max_wgs=cap), ("cap", cap, kind))
    print(WORST["walk"].line(f"{B} images of {H}x{W}"))


_PTRS = ("y", "t", "dy", "dt")
ALIGN_CASES = ([(f"{p}+{o}", tuple(o if q == p else 0 for q in _PTRS)) for p in _PTRS for o in (1, 2, 3)] +
               [(f"all+{o}", (o, o, o, o)) for o in (1, 2, 3)] + [("mixed", (1, 2, 3, 0))])


@pytest.mark.parametrize("label,offs", ALIGN_CASES, ids=[c[0] for c in ALIGN_CASES])
def test_alignment(label, offs):
    """Each pointer 1 to 3 floats off 16-byte alignment, alone and together: the float-at-a-time path, the aligned bits."""
    y, t = WC.inputs(40, 40, 7)
    for kind, param, fw, thr in (("l1", None, 4.0, 0.5), ("charbonnier", 1e-3, 0.0, 0.0)):
        ref = WC.reference(40, 40, 7, "fractional", "sum", kind, param, fw, thr)
        base = WC.launch_ps(y, t, ref["s"], kind, param, fw, thr)
        _same(base, WC.launch_ps(y, t, ref["s"], kind, param, fw, thr, offs=offs), (label, kind))
        prior = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)) * ref["dy"].abs().max().float()
        a = WC.launch_ps(y, t, ref["s"], kind, param, fw, thr, want=("pix", "dy"), dy_scale=-0.25, accumulate=1, prior=prior)
        b = WC.launch_ps(y, t, ref["s"], kind, param, fw, thr, want=("pix", "dy"), dy_scale=-0.25, accumulate=1, prior=prior,
                         offs=offs)
        _same(a, b, (label, kind, "accumulate"))


@pytest.mark.parametrize("kind,param,fw,thr", WC.PARAMS, ids=[f"{k}-{p}-{w}" for k, p, w, _ in WC.PARAMS])
def test_unit_scale_is_the_flat_launch(kind, param, fw, thr):
    """s NULL and s == 1: dy and dt bit for bit tsr_pixel_loss_fwd_bwd's, the summed value within 2^-23 of its loss."""
    for (H, W, B) in ((40, 40, 7), (5, 7, 67), (100, 100, 1)):
        y, t = WC.inputs(H, W, B)
        prior = torch.randn(y.shape, generator=torch.Generator().manual_seed(4)) * 1e-3
        for dy_scale, acc in ((1.0, 0), (-0.25, 0), (-0.25, 1), (1.0, 1)):
            pr = prior.cuda().clone() if acc else None
            loss, dy, dt = Fh.pixel_loss_fwd_bwd(y.cuda(), t.cuda(), kind, param, fw, thr, dy=pr, dy_scale=dy_scale,
                                                 accumulate=bool(acc), want_dt=True)
            for s in (None, torch.ones(B)):
                got = WC.launch_ps(y, t, s, kind, param, fw, thr, dy_scale=dy_scale, accumulate=acc, prior=prior if acc else None)
                lab = (H, W, B, dy_scale, acc, s is None)
                assert torch.equal(bits(got["dy"]), bits(dy.cpu())), lab
                assert torch.equal(bits(got["dt"]), bits(dt.cpu())), lab
                total = float(got["pix"].double().mean())
                assert abs(total - float(loss)) <= 2.0 ** -23 * abs(float(loss)), (lab, total, float(loss))


@pytest.mark.parametrize("name", ["w11_5x40x40", "g_4x40x40", "w11_3x11x12"])
def test_unit_scale_ssim_is_the_parent_launch(name):
    ref = SC.reference(name, "clamped")
    y, t, win, sigma = ref["y"], ref["t"], ref["win"], ref["sigma"]
    B = y.shape[0]
    prior = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)) * 1e-3
    for want_dy, dy_scale, acc in ((False, 1.0, 0), (True, 1.0, 0), (True, -0.25, 1), (True, 0.0, 0)):
        kw = dict(want_dy=want_dy, dy_scale=dy_scale, accumulate=acc, prior=prior if acc else None)
        parent = WC.launch_ssim(y, t, None, win, sigma, ref["C1"], ref["C2"], parent=True, **kw)
        for s in (None, torch.ones(B)):
            _same(parent, WC.launch_ssim(y, t, s, win, sigma, ref["C1"], ref["C2"], **kw), (name, dy_scale, acc, s is None))


@pytest.mark.parametrize("kind,param,fw,thr", [("mse", None, 0.0, 0.0), ("l1", None, 4.0, 0.5), ("charbonnier", 1e-3, 4.0, 0.5),
                                               ("huber", 0.25, 0.0, 0.0)])
def test_unlabeled_samples_are_never_read(kind, param, fw, thr):
    """Weights in {0, 1}, NaN and Inf filling y and t of the zero-weight samples."""
    for (H, W, B) in ((40, 40, 7), (5, 7, 67)):
        y, t = WC.inputs(H, W, B)
        ref = WC.reference(H, W, B, "binary", "sum", kind, param, fw, thr)
        s, skip = ref["s"], ~WC.kept(ref["s"])
        assert skip.any() or B == 1
        yp, tp = WC.poisoned(y, t, s)
        clean = WC.launch_ps(y, t, s, kind, param, fw, thr)
        dirty = WC.launch_ps(yp, tp, s, kind, param, fw, thr)
        _same(clean, dirty, (H, W, B, kind))
        WC.check(ref, dirty["pix"], dirty["dy"], dirty["dt"], label=(H, W, B, kind))
        assert (dirty["pix"][skip] == 0).all() and (dirty["dy"][skip] == 0).all() and (dirty["dt"][skip] == 0).all()
        prior = torch.randn(y.shape, generator=torch.Generator().manual_seed(8)) * ref["dy"].abs().max().float()
        acc_c = WC.launch_ps(y, t, s, kind, param, fw, thr, want=("pix", "dy"), accumulate=1, prior=prior, dy_scale=-0.25)
        acc_d = WC.launch_ps(yp, tp, s, kind, param, fw, thr, want=("pix", "dy"), accumulate=1, prior=prior, dy_scale=-0.25)
        _same(acc_c, acc_d, (H, W, B, kind, "accumulate"))
        WC.check(ref, acc_d["pix"], acc_d["dy"], dy_scale=-0.25, prior=prior, accumulate=True, label=(H, W, B, kind, "accumulate"))
        assert torch.equal(bits(acc_d["dy"][skip]), bits(prior[skip]))


@pytest.mark.parametrize("name", ["w11_5x40x40", "g_4x40x40"])
def test_ssim_ps_weights_and_unlabeled_samples(name):
    ref = SC.reference(name, "clamped")
    y, t, win, sigma, C = ref["y"], ref["t"], ref["win"], ref["sigma"], (ref["C1"], ref["C2"])
    B = y.shape[0]
    s = torch.tensor([1.0, 0.0, 1.75, 0.0, 0.5])[:B]
    skip = ~WC.kept(s)
    yp, tp = WC.poisoned(y, t, s)
    parent = WC.launch_ssim(y, t, None, win, sigma, *C, parent=True)
    got = WC.launch_ssim(yp, tp, s, win, sigma, *C, dy_scale=-0.2)
    _same(got, WC.launch_ssim(y, t, s, win, sigma, *C, dy_scale=-0.2), name)
    assert (got["ssim"][skip] == 0).all() and (got["dy"][skip] == 0).all()
    assert torch.equal(bits(got["ssim"][~skip]), bits(parent["ssim"][~skip]))      # a value is the sample's own
    one = s == 1
    scaled = WC.launch_ssim(y, t, None, win, sigma, *C, dy_scale=-0.2, parent=True)
    assert torch.equal(bits(got["dy"][one]), bits(scaled["dy"][one]))
    want = -WC.f32(0.2) * s.double().view(-1, 1, 1, 1) * ref["g64"]
    err = (got["dy"].double() - want)[~skip].abs().amax(dim=(1, 2, 3))
    fr = WC.frac(err, want[~skip].abs().amax(dim=(1, 2, 3)))
    WORST["ssim"].take({"dy": fr})
    assert fr <= WC.BAR, fr
    prior = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)) * float(want.abs().max())
    acc = WC.launch_ssim(yp, tp, s, win, sigma, *C, dy_scale=-0.2, accumulate=1, prior=prior)
    assert torch.equal(bits(acc["dy"][skip]), bits(prior[skip]))    # untouched
    err = (acc["dy"].double() - prior.double() - want)[~skip].abs().amax(dim=(1, 2, 3))
    assert WC.frac(err, want[~skip].abs().amax(dim=(1, 2, 3))) <= WC.BAR
    vals_only = WC.launch_ssim(yp, tp, s, win, sigma, *C, want_dy=False)
    assert torch.equal(bits(vals_only["ssim"]), bits(got["ssim"]))
    print(WORST["ssim"].line(name))


def test_all_zero_weights_give_zero():
    sref = SC.reference("w11_5x40x40", "clamped")
    y, t = sref["y"].cuda(), torch.full_like(sref["t"], NAN).cuda()
    w = torch.zeros(5).cuda()
    for norm in WC.NORMS:
        loss, dy, pix, vals, pix_b, s, stats = Fh.sr_loss_fwd_bwd(y, t, 0.1, data_range=sref["data_range"], return_parts=True,
                                                                  pixel_kind="l1", sample_weight=w, sample_weight_norm=norm)
        for x in (loss, dy, pix, vals, pix_b, s, stats):
            assert (x == 0).all(), norm
    got = WC.launch_ps(sref["y"], torch.full_like(sref["t"], NAN), torch.zeros(5), "mse")
    assert all((v == 0).all() for v in got.values())


def test_invalid_weights_poison_their_own_sample():
    B = WC.INVALID_B
    y, t = WC.inputs(5, 7, B)
    w = WC.weights_for(B, "invalid", seed=1)
    bad = ~WC.valid(w)
    assert int(bad.sum()) == 4
    for norm in WC.NORMS:
        dev = WC.launch_scale(w, norm)
        s, D, n = WC.scale_ref(w, norm)
        assert torch.isnan(dev["s"][bad]).all() and torch.equal(bits(dev["s"][~bad]), bits(s[~bad])), norm
        assert float(dev["stats"][0]) == WC.f32(D) and float(dev["stats"][1]) == n
        w0 = torch.where(bad, torch.zeros(B), w)                    # the same D without them
        clean_s = WC.launch_scale(w0, norm)["s"]
        assert torch.equal(bits(clean_s[~bad]), bits(dev["s"][~bad])) and (clean_s[bad] == 0).all()
        got = WC.launch_ps(y, t, dev["s"], "huber", 0.25, 4.0, 0.5)
        clean = WC.launch_ps(y, t, clean_s, "huber", 0.25, 4.0, 0.5)
        for k in ("dy", "dt"):
            assert torch.isnan(got[k][bad]).all(), (norm, k)
            assert torch.equal(bits(got[k][~bad]), bits(clean[k][~bad])), (norm, k)
        assert torch.equal(bits(got["pix"][~bad]), bits(clean["pix"][~bad])) and torch.isfinite(got["pix"][bad]).all()
        assert math.isnan(float(WC.launch_mean(got["pix"], dev["s"])))
        assert float(WC.launch_mean(clean["pix"], clean_s)) == WC.mean_ref(clean["pix"], clean_s)


@pytest.mark.parametrize("kind,param", WC.KINDS)
def test_dy_contract(kind, param):
    y, t = WC.inputs(40, 40, 7)
    ref = WC.reference(40, 40, 7, "fractional", "sum", kind, param, 4.0, 0.5)
    s = ref["s"]
    full = WC.launch_ps(y, t, s, kind, param, 4.0, 0.5)
    only = WC.launch_ps(y, t, s, kind, param, 4.0, 0.5, want=("pix",))        # dy = NULL, dt = NULL: the values only
    assert torch.equal(bits(only["pix"]), bits(full["pix"]))
    prior = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)) * ref["dy"].abs().max().float()
    for c in (1.0, -0.25, 0.0):
        got = WC.launch_ps(y, t, s, kind, param, 4.0, 0.5, dy_scale=c)       # overwrite: the NaN prefill is gone
        assert torch.equal(bits(got["pix"]), bits(full["pix"]))
        WC.check(ref, got["pix"], got["dy"], got["dt"], WORST["dy"], dy_scale=c, label=(kind, c))
        if c == 0.0:
            assert (got["dy"] == 0).all() and (got["dt"] == 0).all()
        acc = WC.launch_ps(y, t, s, kind, param, 4.0, 0.5, want=("pix", "dy", "dt"), dy_scale=c, accumulate=1, prior=prior)
        WC.check(ref, acc["pix"], acc["dy"], acc["dt"], WORST["dy"], dy_scale=c, prior=prior, accumulate=True,
                 label=(kind, c, "accumulate"))
        if c == 0.0:
            assert torch.equal(bits(acc["dy"]), bits(prior))
    print(WORST["dy"].line(f"dy contract, {kind}"))


@pytest.mark.parametrize("B", [1, 7, 67, 600, 2048, 4100, 8192])
def test_scale_and_weighted_mean_at_one_rounding(B):
    g = torch.Generator().manual_seed(B)
    v = torch.randn(B, generator=g) * 3 + 1
    for pattern in ("ones", "zeros", "binary", "fractional"):
        w = WC.weights_for(B, pattern, seed=B)
        for norm in WC.NORMS:
            dev = WC.launch_scale(w, norm)
            s, D, n = WC.scale_ref(w, norm)
            assert torch.equal(bits(dev["s"]), bits(s)), (pattern, norm)
            assert float(dev["stats"][0]) == WC.f32(D) and float(dev["stats"][1]) == n, (pattern, norm)
            if pattern == "ones":
                assert (dev["s"] == 1).all()
        s = WC.scale_ref(w, "sum")[0]
        vp = torch.where(WC.kept(s), v, torch.full((B,), NAN))     # a NaN in a skipped entry is never touched
        got = float(WC.launch_mean(vp, s))
        assert got == WC.mean_ref(v, s), (pattern, got)
    assert float(WC.launch_mean(v, None)) == WC.mean_ref(v, None)   # s NULL: the plain mean
    assert float(Fh.weighted_mean(v.cuda())) == WC.mean_ref(v, None)


def _real_buffers(names, n=256):
    return {k: WC.placed(n) for k in names}


def _untouched(bufs):
    return all(bool(torch.isnan(b[0]).all()) for b in bufs.values())


def test_refusal_matrix_leaves_the_buffers_untouched():
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def run(call, base, table, names, want):
        for label, over in table:
            a = dict(base, **over)
            bufs = _real_buffers(names)
            ptrs = {k: (bufs["dy"][1].data_ptr() if a[k] == "dy" else (bufs[k][1].data_ptr() if a[k] else 0)) for k in names}
            st = call(lib, a, stream=stream, **ptrs)
            torch.cuda.synchronize()
            assert st == want, (label, st)
            if want == 1:
                assert _untouched(bufs), label
    ps = dict(WC.PS_BASE, B=2, P=64)
    run(WC.call_ps, ps, WC.PS_REFUSALS, ("y", "t", "s", "pix", "dy", "dt"), 1)
    run(WC.call_ssim_ps, WC.SSIM_BASE, WC.SSIM_REFUSALS, ("y", "t", "s", "ssim", "dy"), 1)
    run(WC.call_scale, WC.SCALE_BASE, WC.SCALE_REFUSALS, ("w", "s", "stats"), 1)
    run(WC.call_mean, WC.MEAN_BASE, WC.MEAN_REFUSALS, ("v", "s", "out"), 1)
    for label, over in WC.PS_ACCEPTED:                              # and what the table must not refuse
        a = dict(ps, **over)
        bufs = {k: WC.placed(256, fill=torch.ones(256)) for k in ("y", "t", "s", "pix", "dy", "dt")}
        ptrs = {k: (bufs[k][1].data_ptr() if a[k] else 0) for k in bufs}
        assert WC.call_ps(lib, a, stream=stream, **ptrs) == 0, label
        torch.cuda.synchronize()


def test_functional_forms():
    y, t = (x.view(7, 1, 40, 40) for x in WC.inputs(40, 40, 7))
    ref = WC.reference(40, 40, 7, "fractional", "sum", "huber", 0.25, 4.0, 0.5)
    w = WC.weights_for(7, "fractional", seed=7)
    s, stats = Fh.sample_scale(w.cuda())
    assert torch.equal(bits(s.cpu()), bits(ref["s"])) and float(stats[0]) == WC.f32(WC.scale_ref(w, "sum")[1])
    pix, dy, dt = Fh.pixel_loss_per_sample(y.cuda(), t.cuda(), "huber", 0.25, 4.0, 0.5, scale=s, want_dt=True)
    WC.check(ref, pix.cpu(), dy.cpu(), dt.cpu(), label="functional")
    p3, d3 = Fh.pixel_loss_per_sample(y.cuda(), t.cuda(), "huber", 0.25, 4.0, 0.5, scale=s, max_wgs=3)
    assert torch.equal(p3, pix) and torch.equal(d3, dy)
    for bad in (dict(scale=s[:3]), dict(scale=s.cpu()), dict(accumulate=True), dict(dy=torch.empty(3, device="cuda")),
                dict(kind="l3"), dict(max_wgs=0)):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.pixel_loss_per_sample(y.cuda(), t.cuda(), **{"kind": "mse", **bad})
    with pytest.raises(_lib.TactileSRHipError):
        Fh.sample_scale(w.cuda(), "mean")
    # no weight: exactly today's launches and bits
    sref = SC.reference("w11_5x40x40", "clamped")
    ys, ts = sref["y"].cuda(), sref["t"].cuda()
    a = Fh.sr_loss_fwd_bwd(ys, ts, 0.1, return_parts=True, pixel_kind="l1")
    b = Fh.sr_loss_fwd_bwd(ys, ts, 0.1, return_parts=True, pixel_kind="l1", sample_weight=None, sample_weight_norm="batch")
    assert len(a) == len(b) == 4 and all(torch.equal(u, v) for u, v in zip(a, b))
    # all ones: the same gradient bit for bit, the same loss to the bar
    c = Fh.sr_loss_fwd_bwd(ys, ts, 0.1, return_parts=True, pixel_kind="l1", sample_weight=torch.ones(5).cuda())
    assert len(c) == 7 and torch.equal(bits(c[1]), bits(a[1])) and torch.equal(c[3], a[3])
    assert abs(float(c[0]) - float(a[0])) <= 1e-6 * float(a[0]) and c[4].shape == (5,)


# ------------------------------------------------------------------------------------------------------------ the train step
def _model(impl, seed=42):
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR(10, 1, 3, 1, 1).cuda().train()
    m.train_impl = impl
    return m


W4 = (1.0, 0.0, 1.0, 0.5)


def _batch(B=4, seed=11, weights=W4, poison=True):
    """Random taxels, a contact-like HR (blobs of amplitude <= 100 raw) and the weights; the HR of every zero-weight sample
    is NaN."""
    g = torch.Generator().manual_seed(seed)
    LR, HR = torch.rand(B, 3, 4, 4, generator=g) * 8, SC.blobs(B, 100, 100, g) * 10
    w = torch.tensor(weights, dtype=torch.float32)
    if poison:
        HR[w == 0] = NAN
    return LR.cuda(), HR.cuda(), None, w.cuda()


LAM, GAMMA = 0.1, 0.7
BASE = TR.default_config()
TRAIN_CONFS = {"alone": BASE, "ssim": dict(BASE, ssim_loss_weight=0.1, ssim_data_range=10.0),
               "degradation": dict(BASE, degradation_loss_weight=LAM, degradation_gamma=GAMMA)}


def _loss64(out, HR, LR, w, conf):
    """The configured weighted loss in fp64 on the host from the device's output (autograd crosses the copy)."""
    o, h = out.double().cpu(), HR.double().cpu()
    s, D, _ = WC.scale_ref(w.cpu(), TR.sample_weight_config(conf))
    name, p, fw, thr = TR.pixel_loss_config(conf)
    lam_s, window, sigma, rng = TR.ssim_loss_config(conf)
    loss, pix = WC.restatement(o, h, s, name, p, fw, thr, lam_s, (window, sigma, *SC.constants(rng)))
    w_d, gamma, ch, gain = TR.degradation_loss_config(conf)
    if w_d:
        loss = loss + w_d * DC.restatement(o, LR[:, ch].double().cpu().reshape(-1, 16), gamma, gain)[1].mean()
    return loss, float((s.double() * pix.detach())[WC.kept(s)].sum() / o.shape[0]), D / o.shape[0]


@pytest.mark.parametrize("norm", list(WC.NORMS))
@pytest.mark.parametrize("name", list(TRAIN_CONFS))
def test_train_cal_loss_fp16x3_against_fp64(name, norm):
    conf = dict(TRAIN_CONFS[name], sample_weight_norm=norm)
    batch = _batch()
    m = _model("fp16x3")
    loss, parts = TR.train_cal_loss(m, batch, conf)
    assert set(parts) == ({"total_loss", "mse_loss", "labeled_weight"} | ({"ssim"} if name == "ssim" else set()) |
                          ({"degradation_loss"} if name == "degradation" else set()))
    m.zero_grad()
    loss.backward()
    r = _model("fp16x3")
    LR, HR = TR._prep(batch, conf, "cuda")
    assert torch.isnan(HR[1]).all()                                 # the unlabeled sample's target is NaN on the device
    out = r(LR)
    loss64, pix64, labeled = _loss64(out, HR, LR, batch[3], conf)
    r.zero_grad()
    loss64.backward()
    l64 = float(loss64.detach())
    assert math.isfinite(l64) and abs(float(loss.detach()) - l64) <= 1e-5 * abs(l64), (float(loss.detach()), l64)
    assert abs(float(parts["mse_loss"]) - pix64) <= 1e-5 * pix64
    assert abs(float(parts["labeled_weight"]) - labeled) <= 1e-6 * labeled and labeled == 2.5 / 4
    want = {n: p.grad.detach().cpu().double() for n, p in r.named_parameters()}
    worst = _gradcheck.check_grads({n: p.grad for n, p in m.named_parameters()}, want, tol=2e-5)
    print(f"[sample weight] train_cal_loss fp16x3 {name} {norm}: loss {float(loss.detach()):.6f}, worst parameter gradient "
          f"{worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("norm", list(WC.NORMS))
@pytest.mark.parametrize("name", list(TRAIN_CONFS))
def test_train_cal_loss_bf16_is_the_engine_backward_of_the_launch(name, norm):
    conf = dict(TRAIN_CONFS[name], sample_weight_norm=norm)
    batch = _batch()
    m = _model("bf16")
    loss, parts = TR.train_cal_loss(m, batch, conf)
    m.zero_grad()
    loss.backward()
    r = _model("bf16")
    LR, HR = TR._prep(batch, conf, "cuda")
    out = r(LR)
    lam_s, window, sigma, rng = TR.ssim_loss_config(conf)
    kind, param, fw, thr = TR.pixel_loss_config(conf)
    w_d, gamma, ch, gain = TR.degradation_loss_config(conf)
    l2, dy = Fh.sr_loss_fwd_bwd(out.detach().float(), HR, lam_s, rng, window, sigma, pixel_kind=kind, pixel_param=param,
                                fg_weight=fw, fg_threshold=thr, deg_weight=w_d, deg_z=LR[:, ch] if w_d else None,
                                deg_gamma=gamma, deg_gain=gain or 1.0, sample_weight=batch[3], sample_weight_norm=norm)
    assert (dy[1] == 0).all() or w_d
    r.zero_grad()
    out.backward(dy.to(out.dtype))
    assert torch.equal(loss.detach(), l2[0]) and math.isfinite(float(loss.detach()))
    for (n, a), (_, b) in zip(m.named_parameters(), r.named_parameters()):
        assert torch.equal(bits(a.grad), bits(b.grad)), n


def test_an_all_unlabeled_batch_trains_on_the_degradation_term_alone():
    conf = TRAIN_CONFS["degradation"]
    batch = _batch(weights=(0.0, 0.0, 0.0, 0.0))
    m = _model("bf16")
    loss, parts = TR.train_cal_loss(m, batch, conf)
    m.zero_grad()
    loss.backward()
    assert float(parts["mse_loss"]) == 0 and float(parts["labeled_weight"]) == 0
    assert float(loss.detach()) == WC.f32(WC.f32(LAM) * float(parts["degradation_loss"])) > 0      # 0 + one fp32 product
    r = _model("bf16")
    LR, HR = TR._prep(batch, conf, "cuda")
    out = r(LR)
    q, _, dy = Fh.degradation_fwd_bwd(out.detach().float(), LR[:, 2], GAMMA, 10.0, dy_scale=LAM / 4)
    r.zero_grad()
    out.backward(dy.to(out.dtype))
    assert torch.equal(q.mean(), parts["degradation_loss"])
    for (n, a), (_, b) in zip(m.named_parameters(), r.named_parameters()):
        assert torch.equal(bits(a.grad), bits(b.grad)), n
    assert max(float(p.grad.abs().max()) for p in m.parameters()) > 0
    with pytest.raises(_lib.TactileSRHipError):                     # no gamma anywhere
        TR.train_cal_loss(m, batch, dict(BASE, degradation_loss_weight=LAM))


def test_unit_weights_send_the_unweighted_gradient():
    """A 4-tuple of ones under the configured pixel launch and the SSIM term: dy is the 2-tuple step's bit for bit."""
    conf = dict(BASE, pixel_loss="l1", ssim_loss_weight=0.1, ssim_data_range=10.0)
    LR, HR, _, _ = _batch(poison=False)
    a, b = _model("bf16"), _model("bf16")
    la, pa = TR.train_cal_loss(a, (LR, HR), conf)
    lb, pb = TR.train_cal_loss(b, (LR, HR, None, torch.ones(4)), conf)      # a CPU weight is moved with the batch
    la.backward()
    lb.backward()
    assert set(pb) == set(pa) | {"labeled_weight"} and float(pb["labeled_weight"]) == 1
    for k in pa:
        assert abs(float(pa[k]) - float(pb[k])) <= 1e-6 * abs(float(pa[k])), k
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(bits(p.grad), bits(q.grad)), n


def _same_state(ma, oa, mb, ob):
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]), n
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    for (n, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(a, b), n


def test_graphed_step_takes_the_weights_as_data():
    conf = dict(BASE, ssim_loss_weight=0.1, ssim_data_range=10.0, degradation_loss_weight=LAM, degradation_gamma=GAMMA)
    weights = [W4, (0.0, 2.0, 0.25, 0.0), (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), (0.5, 0.0, 0.0, 3.0), (0.0, 1.0, 1.0, 0.0)]
    batches = [_batch(seed=20 + i, weights=w) for i, w in enumerate(weights)]
    me, mg = _model("fp16x3"), _model("fp16x3")
    oe = optim.Adam(me.parameters(), lr=1e-3, weight_decay=1e-2)
    og = optim.Adam(mg.parameters(), lr=1e-3, weight_decay=1e-2)
    gconf = copy.deepcopy(conf)
    gstep = GraphedTrainStep(mg, og, gconf, warmup=1)
    for i, b in enumerate(batches[:4]):                             # one eager warm-up step, then three replays
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert set(pe) == set(pg) == {"total_loss", "mse_loss", "ssim", "degradation_loss", "labeled_weight"}
        for k in pe:
            assert torch.equal(pe[k].detach(), pg[k]), (i, k, float(pe[k]), float(pg[k]))
            assert math.isfinite(float(pg[k])), (i, k)
    assert gstep.captures == 1
    _same_state(me, oe, mg, og)
    with pytest.raises(_lib.TactileSRHipError):                     # the signature holds the weight
        gstep(batches[4][:2])
    conf["sample_weight_norm"] = gconf["sample_weight_norm"] = "batch"      # a baked constant: dropped and recaptured
    for i, b in enumerate(batches[4:]):
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        for k in pe:
            assert torch.equal(pe[k].detach(), pg[k]), (i, k)
    assert gstep.captures == 2
    _same_state(me, oe, mg, og)


def test_eval_func_with_weights():
    m = _model("fp16x3")
    conf = dict(BASE, degradation_gamma=GAMMA)
    g = torch.Generator().manual_seed(5)

    def loader(B, n):
        out = []
        for i in range(n):
            w = WC.weights_for(B, "fractional", seed=40 + i)
            out.append(_batch(B, seed=31 + i, weights=w.tolist()))
        return out
    for ld in (loader(8, 2), loader(3, 3)):
        plain = [(b[0], torch.nan_to_num(b[1], nan=1.0)) for b in ld]
        five = TR.eval_func(m, ld, conf, windowed_ssim=True, degradation=True)
        assert len(five) == 5 and all(math.isfinite(v) for v in five)
        assert five[4] == TR.eval_func(m, plain, conf, degradation=True)[3]      # the plain mean over all samples
        tot = [0.0] * 4
        tw = 0.0
        with torch.no_grad():
            for b in ld:
                LR, HR = TR._prep(b, conf, "cuda")
                out = m(LR)
                keep = (b[3] != 0).cpu()
                o, h, w = out[keep].double().cpu(), HR[keep].double().cpu(), b[3][keep].double().cpu()
                ps, ss = Fh.psnr_ssim(out[keep], HR[keep], conf["sensorMaxVaule_factor"], reference_quirk=True)
                ws = SC.restatement(o, h, 11, 1.5, *SC.constants(1.0))
                for k, mval in enumerate((((o - h) ** 2).mean(dim=(1, 2, 3)), ss.double().cpu(), ps.double().cpu(), ws)):
                    tot[k] += float((w * mval).sum())
                tw += float(w.sum())
        for got, want in zip(five[:4], tot):
            assert abs(got - want / tw) <= 1e-5 * abs(want / tw), (got, want / tw)
    zero = [_batch(3, seed=50, weights=(0.0, 0.0, 0.0))]
    none = TR.eval_func(m, zero, conf, windowed_ssim=True, degradation=True)
    assert all(v != v for v in none[:4]) and math.isfinite(none[4])
    m.train()


def test_one_epoch_from_a_weighted_loader():
    g = torch.Generator().manual_seed(9)
    n = 21
    LR, HR = torch.rand(n, 3, 4, 4, generator=g) * 8, SC.blobs(n, 100, 100, g)[:, 0] * 10
    w = WC.weights_for(n, "fractional", seed=4) + torch.where(torch.arange(n) % 5 == 4, 0.0, 1.0) * torch.arange(n) * 4.0
    HR[w == 0] = NAN
    ld = DeviceSRLoader(LR, HR, 4, shuffle=True, seed=3, device="cuda", augment="dihedral", taxel_noise=dict(sigma_add=0.02),
                        weight=w)
    m = _model("fp16x3")
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    conf = dict(BASE, ssim_loss_weight=0.1, ssim_data_range=10.0, degradation_loss_weight=LAM, degradation_gamma=GAMMA)
    seen = []
    for lr, hr, gm, ww in ld:
        assert gm is None and ww.is_cuda and ww.dtype == torch.float32 and torch.equal(ww.cpu(), w[ld.last_index.cpu()])
        assert torch.equal(torch.isnan(hr).flatten(1).all(dim=1).cpu(), ww.cpu() == 0)      # the NaN HR travels with its weight
        parts = TR.train_one_iter(m, opt, (lr, hr.unsqueeze(1), None, ww), conf)
        assert all(math.isfinite(float(v)) for v in parts.values()), parts
        seen += ld.last_index.tolist()
    assert sorted(seen) == list(range(n))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
