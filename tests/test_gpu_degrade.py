"""GPU checks of the degradation-consistency loss (tsr_degrade_fwd_bwd, functional.degrade / degradation_fwd_bwd /
degradation_loss / sr_loss_fwd_bwd, the degradation keys of train_cal_loss, GraphedTrainStep and eval_func, the loader's
gamma) against the fp64 restatement and THE RULE of tests/_degrade_cases.py: |kernel - fp64| <= 1e-5 x the image's own
maximum of the quantity.  Every output buffer is prefilled with NaN between NaN guard bands, and every launch runs twice
and must give the same bits."""
import copy
import math

import pytest
import torch

import _degrade_cases as DC
import _gradcheck
import _pixel_loss_cases as PC
import _ssim_cases as SC
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib, optim
from tactilesr_amd.data.device_loader import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

pytestmark = pytest.mark.gpu

NAN, INF = DC.NAN, DC.INF
bits = DC.bits
WORST = {k: DC.Worst() for k in ("shapes", "gamma", "impulse", "walk", "align", "dy", "golden", "autograd")}


def _same(a, b, what=""):
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("H,W", list(DC.SHAPES), ids=[f"{h}x{w}" for h, w in DC.SHAPES])
def test_shapes(H, W):
    """(a)"""
    for B in DC.BATCHES:
        for signed in (False, True):
            for gamma in DC.GAMMAS:
                for gain in DC.GAINS:
                    ref = DC.reference(H, W, B, signed, gamma, gain)
                    out = DC.launch(ref["y"], ref["z"], gamma, gain)
                    DC.check(ref, **out, worst=WORST["shapes"], label=(H, W, B, signed, gamma, gain))
    print(WORST["shapes"].line(f"shapes, up to {H}x{W}"))


@pytest.mark.parametrize("H,W,B", [(40, 40, 67), (100, 100, 7), (5, 7, 67)])
def test_per_sample_gamma(H, W, B):
    """(b)"""
    g = DC.per_sample_gammas(B, seed=H)
    ref = DC.build_reference(DC.images(H, W, B, False), g, 10.0, seed=1)
    out = DC.launch(ref["y"], ref["z"], g, 10.0)
    DC.check(ref, **out, worst=WORST["gamma"], label=("per-sample gamma", H, W))
    for gamma in (0.7, 0.05):                                       # a device gamma equal to the host scalar: the same bits
        g32 = torch.full((B,), gamma, dtype=torch.float32)
        dev = DC.launch(ref["y"], ref["z"], g32, 10.0)
        host = DC.launch(ref["y"], ref["z"], float(g32[0]), 10.0)
        _same(dev, host, ("device gamma == host gamma", gamma))
    print(WORST["gamma"].line(f"per-sample gamma, up to {H}x{W}"))


@pytest.mark.parametrize("H,W", [(5, 7), (40, 40), (100, 100), (128, 128)])
def test_impulses(H, W):
    """(c)"""
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    if (H, W) == (100, 100):
        pos += [(12 + 25 * a, 12 + 25 * c) for a in range(4) for c in range(4)]
    y = torch.zeros(len(pos), 1, H, W)
    for b, (i, j) in enumerate(pos):
        y[b, 0, i, j] = 3.0 + b
    for gamma in DC.GAMMAS:
        for gain in DC.GAINS:
            ref = DC.build_reference(y, gamma, gain, z=torch.full((len(pos), 16), 1e-4))
            out = DC.launch(y, ref["z"], gamma, gain)
            assert float(ref["D"].abs().amax(dim=1).min()) > 1e-30      # every pooled impulse is a normal fp32 number
            DC.check(ref, **out, worst=WORST["impulse"], label=("impulse", H, W, gamma, gain))
            assert torch.isfinite(out["lr_deg"]).all() and torch.isfinite(out["dy"]).all()
            if (H, W) == (100, 100):                                # at a taxel centre D = gain 1e-4 v, to one rounding
                for b in range(4, 20):
                    want = float(torch.tensor(gain * 1e-4 * (3.0 + b), dtype=torch.float32))
                    got = float(out["lr_deg"][b, b - 4])
                    assert abs(got - want) <= 2.0 ** -23 * want, (gamma, gain, b, got, want)
    print(WORST["impulse"].line(f"impulses, {H}x{W}"))


@pytest.mark.parametrize("H,W", [(5, 7), (40, 40)])
def test_zero_image_is_exact(H, W):
    """(d)"""
    B = 5
    y = torch.zeros(B, 1, H, W)
    z = torch.randn(B, 16, generator=torch.Generator().manual_seed(3))
    for gamma in DC.GAMMAS:
        out = DC.launch(y, z, gamma, 10.0)
        assert (out["lr_deg"] == 0).all() and torch.equal(bits(out["dz"]), bits(z * 0.125))       # r = -z exactly
        q64 = (z.double() ** 2).mean(dim=1)
        assert float(((out["q"].double() - q64).abs() / q64).max()) <= DC.BAR
        ref = DC.build_reference(y, gamma, 10.0, z=z)
        DC.check(ref, dy=out["dy"], label=("zero image", gamma))


def test_batch_walk():
    """(e)"""
    B = 2100
    assert B > DC.MAX_WGS
    y = DC.images(12, 20, B, False)
    assert len({float(v) for v in y.sum(dim=(1, 2, 3))}) == B      # distinct images
    for gamma in (DC.per_sample_gammas(B, seed=8), 0.7):
        ref = DC.build_reference(y, gamma, 10.0, seed=2)
        full = DC.launch(y, ref["z"], gamma, 10.0)
        DC.check(ref, **full, worst=WORST["walk"], label="walk, the default cap")
        for cap in (1, 3):
            _same(DC.launch(y, ref["z"], gamma, 10.0, max_wgs=cap), full, ("cap", cap))
    print(WORST["walk"].line("2100 images, caps 1 / 3 / default"))


_OFFS = ([(f"y+{o}", (o, 0, 0)) for o in (1, 2, 3)] + [(f"dy+{o}", (0, o, 0)) for o in (1, 2, 3)] +
         [(f"z+{o}", (0, 0, o)) for o in (1, 2, 3)] + [(f"all+{o}", (o, o, o)) for o in (1, 2, 3)] + [("mixed", (1, 2, 3))])


@pytest.mark.parametrize("label,offs", _OFFS, ids=[c[0] for c in _OFFS])
def test_alignment_and_stride(label, offs):
    """(f)"""
    ref = DC.reference(40, 40, 7, False, 0.7, 10.0)
    base = DC.launch(ref["y"], ref["z"], 0.7, 10.0)
    prior = torch.ones(ref["y"].shape) * ref["dy"].abs().max().float()
    base_acc = DC.launch(ref["y"], ref["z"], 0.7, 10.0, dy_scale=-0.25, accumulate=1, prior=prior)
    for layout in ((1, 0), (3, 2), (21, 20), (21, 5)):
        out = DC.launch(ref["y"], ref["z"], 0.7, 10.0, offs=offs, z_layout=layout)
        DC.check(ref, **out, worst=WORST["align"], label=(label, layout))
        _same(out, base, (label, layout))                           # an element does not depend on the path
        acc = DC.launch(ref["y"], ref["z"], 0.7, 10.0, dy_scale=-0.25, accumulate=1, prior=prior, offs=offs, z_layout=layout)
        DC.check(ref, **acc, dy_scale=-0.25, prior=prior, worst=WORST["align"], label=(label, layout, "accumulate"))
        _same(acc, base_acc, (label, layout, "accumulate"))
    print(WORST["align"].line(f"alignment and stride, up to {label}"))


@pytest.mark.parametrize("H,W", [(40, 40), (5, 7)])
def test_dy_contract(H, W):
    """(g)"""
    ref = DC.reference(H, W, 7, True, 5.0, 10.0)
    full = DC.launch(ref["y"], ref["z"], 5.0, 10.0)
    for want in (("q",), ("lr_deg", "q"), ("q", "dz"), ("q", "dy")):                 # NULL outputs: the rest keeps its bits
        part = DC.launch(ref["y"], ref["z"], 5.0, 10.0, want=want)
        assert set(part) == set(want)
        _same(part, {k: full[k] for k in want}, want)
    fwd = DC.launch(ref["y"], None, 5.0, 10.0, want=("lr_deg",))                      # z = NULL: the forward alone
    _same(fwd, {"lr_deg": full["lr_deg"]}, "forward alone")
    prior = torch.randn(ref["y"].shape, generator=torch.Generator().manual_seed(5)) * ref["dy"].abs().max().float()
    for s in (1.0, -0.25, 0.0):
        out = DC.launch(ref["y"], ref["z"], 5.0, 10.0, dy_scale=s)                   # accumulate = 0 overwrites the NaN prefill
        DC.check(ref, **out, dy_scale=s, worst=WORST["dy"], label=("overwrite", s))
        _same({k: out[k] for k in ("lr_deg", "q")}, {k: full[k] for k in ("lr_deg", "q")}, s)
        assert torch.equal(bits(out["dz"]), bits(full["dz"] * s)) or s == 0           # dz = -dy_scale r / 8; s a power of two
        if s == 0:
            assert (out["dy"] == 0).all() and (out["dz"] == 0).all()
        acc = DC.launch(ref["y"], ref["z"], 5.0, 10.0, dy_scale=s, accumulate=1, prior=prior)
        DC.check(ref, **acc, dy_scale=s, prior=prior, worst=WORST["dy"], label=("accumulate", s))
        assert torch.equal(bits(acc["dz"]), bits(out["dz"]))                         # dz is overwritten, never accumulated
        if s == 0:
            assert torch.equal(bits(acc["dy"]), bits(prior))
    r64 = ref["D"] - ref["z"].double()                                              # dz == -dy_scale r / 8
    assert float((full["dz"].double() + r64 / 8).abs().max()) <= DC.BAR * float(r64.abs().max()) / 8
    print(WORST["dy"].line(f"dy contract, {H}x{W}"))


def test_non_finite_inputs_stay_in_their_own_image():
    """(h)"""
    B, H, W = 600, 12, 20
    y = DC.images(H, W, B, False).clone()
    g = DC.per_sample_gammas(B, seed=6)
    z = DC.build_reference(y, g, 10.0, seed=4)["z"]
    prior = torch.ones(y.shape)
    clean = DC.launch(y, z, g, 10.0, dy_scale=-0.25, accumulate=1, prior=prior)
    assert all(torch.isfinite(v).all() for v in clean.values())
    yb, gb = y.clone(), g.clone()
    yb[5, 0, 3, 7], yb[9, 0, 11, 0] = NAN, INF
    bad_g = list(range(20, 600, 37))[:16]
    assert len(bad_g) == 16
    for n, i in enumerate(bad_g):
        gb[i] = (0.0, -1.0, NAN, INF, -INF, -0.0, 2e6, 1e18)[n % 8]
    out = DC.launch(yb, z, gb, 10.0, dy_scale=-0.25, accumulate=1, prior=prior)
    keep = torch.ones(B, dtype=torch.bool)
    keep[[5, 9] + bad_g] = False
    for k in out:
        assert torch.equal(bits(out[k][keep]), bits(clean[k][keep])), (k, "a clean image changed")
    for i in (5, 9):                                                # the pixel reaches every taxel and the whole gradient
        assert not torch.isfinite(out["lr_deg"][i]).any() and not math.isfinite(float(out["q"][i]))
        assert not torch.isfinite(out["dy"][i]).any()
    for i in bad_g:                                                 # all-NaN, whatever accumulate says
        assert all(torch.isnan(out[k][i]).all() for k in out), i


def _refusal_call(a):
    B, H, W = max(a["B"], 1), 8, 8
    y = torch.rand(2 * B * H * W, device="cuda")
    z = torch.rand(B * 16, device="cuda")
    g = torch.full((B,), 0.7, device="cuda")
    bufs = {k: DC.placed(n) for k, n in (("lr_deg", 16 * B), ("q", B), ("dy", B * H * W), ("dz", 16 * B))}
    addr = dict(y=y.data_ptr(), z=z.data_ptr(), gamma_dev=g.data_ptr(), **{k: v[1].data_ptr() for k, v in bufs.items()})
    ptrs = {k: (addr[k] if a[k] else 0) for k in addr}
    if a["dy"] == "y":
        ptrs["dy"] = addr["y"]
    elif a["dy"] == "y+":
        ptrs["dy"] = addr["y"] + 4 * H * W
    st = DC.call_raw(_lib.load(), a, stream=torch.cuda.current_stream().cuda_stream, **ptrs)
    torch.cuda.synchronize()
    return st, bufs, y


@pytest.mark.parametrize("label,over", DC.REFUSALS, ids=[r[0] for r in DC.REFUSALS])
def test_refusal_matrix(label, over):
    """(i)"""
    a = dict(DC.BASE_ARGS, **over)
    if a["H"] > 8 or a["W"] > 8:                                    # the refused size is never allocated
        assert DC.call_raw(_lib.load(), a, y=64, z=64, lr_deg=64, q=64, dy=1 << 30, dz=64) == 1
        return
    st, bufs, y = _refusal_call(a)
    assert st == 1, (label, st)
    assert all(torch.isnan(b[0]).all() for b in bufs.values()) and torch.isfinite(y).all(), (label, "a refused call wrote")


@pytest.mark.parametrize("label,over", DC.ACCEPTED, ids=[r[0] for r in DC.ACCEPTED])
def test_the_table_refuses_no_more_than_the_header(label, over):
    a = dict(DC.BASE_ARGS, **over)
    st, bufs, _ = _refusal_call(a)
    assert st == 0, (label, st)
    for k, (buf, mid, start) in bufs.items():
        assert bool(torch.isnan(mid).any()) != bool(a[k]) or (k == "dy" and a["dy_scale"] == INF), (label, k)
        assert DC.guards_intact(buf, start, mid.numel()), (label, k)


def test_golden_file(golden):
    """(j)"""
    g = golden("degrade")
    y, gamma = torch.from_numpy(g["y"])[:, None].contiguous(), torch.from_numpy(g["gamma"])
    ref = DC.build_reference(y, gamma, 1.0)
    out = DC.launch(y, ref["z"], gamma, 1.0)
    DC.check(ref, **out, worst=WORST["golden"], label="golden")
    want = torch.from_numpy(g["lr_deg_f32"]).double()
    err = float(((out["lr_deg"].double() - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max())
    assert err <= 2e-6, err                                         # the reference's own fp32 arithmetic
    dev = Fh.degrade(y.cuda(), gamma.cuda()).cpu()
    assert dev.shape == (6, 1, 4, 4) and torch.equal(bits(dev.view(6, 16)), bits(out["lr_deg"]))
    one = Fh.degrade(y[1:2].cuda(), float(gamma[1])).cpu()
    assert torch.equal(bits(one.view(16)), bits(out["lr_deg"][1]))
    print(WORST["golden"].line(f"golden file (the reference's fp32 outputs are {err:.2e} away)"))


# ------------------------------------------------------------------------------------------------------ functional layer
def test_degradation_loss_backward_to_image_and_taxels():
    """(k)"""
    B = 7
    g = DC.per_sample_gammas(B, seed=12)
    ref = DC.build_reference(DC.images(40, 40, B, True), g, 10.0, seed=9)
    y = ref["y"].cuda().requires_grad_(True)
    z = ref["z"].view(B, 1, 4, 4).cuda().requires_grad_(True)
    loss = Fh.degradation_loss(y, z, g.cuda(), 10.0)
    (0.37 * loss).backward()
    want = float(ref["q"].mean())
    assert abs(float(loss.detach()) - want) <= DC.BAR * want
    DC.check(ref, dy=y.grad.cpu(), dz=z.grad.cpu().view(B, 16), dy_scale=0.37 / B, worst=WORST["autograd"], label="autograd")
    assert z.grad.shape == z.shape
    y2, z2 = ref["y"].cuda().requires_grad_(True), ref["z"].cuda()   # taxels that ask for no gradient get none
    l2 = Fh.degradation_loss(y2, z2, g.cuda(), 10.0)
    (0.37 * l2).backward()
    assert z2.grad is None and torch.equal(l2.detach(), loss.detach()) and torch.equal(y2.grad, y.grad)
    print(WORST["autograd"].line("degradation_loss with an upstream gradient"))


def test_fwd_bwd_arguments_and_the_sr_loss_launch_order():
    B = 5
    sref = SC.reference("w11_5x40x40", "clamped")
    y, t = sref["y"].cuda(), sref["t"].cuda()
    LR = torch.rand(B, 3, 4, 4, generator=torch.Generator().manual_seed(2)).cuda()
    ref = DC.build_reference(sref["y"], 0.7, 10.0, z=LR[:, 2].cpu().reshape(B, 16))
    q, lr_deg, dy, dz = Fh.degradation_fwd_bwd(y, LR[:, 2], 0.7, 10.0, want_dz=True)                  # a channel slice, in place
    DC.check(ref, lr_deg.cpu().view(B, 16), q.cpu(), dy.cpu(), dz.cpu().view(B, 16), label="fwd_bwd")
    qs, ls, none = Fh.degradation_fwd_bwd(y, LR[:, 2], 0.7, 10.0, want_dy=False)                    # a score: no dy at all
    assert none is None and torch.equal(qs, q) and torch.equal(ls, lr_deg)
    for zz in (LR[:, 2:3], LR[:, 2].reshape(B, 16), LR[:, 2].contiguous(), LR[:, 2].double()):
        q2, l2, d2 = Fh.degradation_fwd_bwd(y, zz, 0.7, 10.0)
        assert torch.equal(q2, q) and torch.equal(l2, lr_deg) and torch.equal(d2, dy)
    for bad in (dict(gamma=0.0), dict(gamma=torch.ones(B)), dict(gamma=torch.ones(B + 1, device="cuda")), dict(gain=NAN),
                dict(accumulate=True), dict(dy=torch.empty(3, device="cuda")), dict(dy_scale=NAN), dict(dy=y), dict(gamma=2e6),
                dict(want_dy=False, accumulate=True), dict(want_dy=False, dy=torch.empty_like(y))):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.degradation_fwd_bwd(y, LR[:, 2], **{"gamma": 0.7, **bad})
    with pytest.raises(_lib.TactileSRHipError):
        Fh.degradation_fwd_bwd(y, LR[:3, 2], 0.7)
    # weight 0: today's launches and bits
    l0, d0, p0, v0 = Fh.sr_loss_fwd_bwd(y, t, 0.1, return_parts=True)
    l1, d1, p1, v1 = Fh.sr_loss_fwd_bwd(y, t, 0.1, return_parts=True, deg_weight=0.0, deg_z=LR[:, 2], deg_gamma=0.7)
    assert torch.equal(l0, l1) and torch.equal(d0, d1) and torch.equal(v0, v1)
    # the term accumulates deg_weight / B dq/dy behind the SSIM launch
    lam = 0.3
    loss, dyt, pix, vals, qq = Fh.sr_loss_fwd_bwd(y, t, 0.1, return_parts=True, deg_weight=lam, deg_z=LR[:, 2],
                                                  deg_gamma=0.7, deg_gain=10.0)
    assert torch.equal(qq, q) and torch.equal(pix, p0) and torch.equal(vals, v0)
    assert abs(float(loss) - (float(l0) + lam * float(ref["q"].mean()))) <= DC.BAR * float(loss)
    g64 = d0.cpu().double() + lam / B * ref["dy"]
    err = (dyt.cpu().double() - g64).abs().amax(dim=(1, 2, 3)) / g64.abs().amax(dim=(1, 2, 3))
    assert float(err.max()) <= DC.BAR, err.tolist()
    moved = (dyt - d0).abs().amax() / d0.abs().amax()
    assert float(moved) > 100 * DC.BAR                              # the bar can see the term in the sum


# ------------------------------------------------------------------------------------------------------------ the train step
def _model(impl, seed=42):
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR(10, 1, 3, 1, 1).cuda().train()
    m.train_impl = impl
    return m


def _batch(B=4, seed=11):
    """Random taxels and a contact-like HR: blobs of amplitude <= 100 raw, <= 10 after HR_scale_num."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (SC.blobs(B, 100, 100, g) * 10).cuda()


LAM, GAMMA = 0.1, 0.7
DEG = dict(TR.default_config(), degradation_loss_weight=LAM, degradation_gamma=GAMMA)
TRAIN_CONFS = {"alone": DEG, "ssim": dict(DEG, ssim_loss_weight=0.1, ssim_data_range=10.0),
               "l1": dict(DEG, pixel_loss="l1")}


def _loss64(out, HR, LR, conf):
    """The configured loss in fp64 on the host from the device's output (autograd crosses the copy)."""
    o, h = out.double().cpu(), HR.double().cpu()
    name, p, w, thr = TR.pixel_loss_config(conf)
    loss = PC.restatement(o, h, name, p, w, thr)
    lam_s, window, sigma, rng = TR.ssim_loss_config(conf)
    if lam_s:
        loss = loss + lam_s * (1 - SC.restatement(o, h, window, sigma, *SC.constants(rng)).mean())
    w_d, gamma, ch, gain = TR.degradation_loss_config(conf)
    q = DC.restatement(o, LR[:, ch].double().cpu().reshape(-1, 16), gamma, gain)[1]
    return loss + w_d * q.mean(), q


@pytest.mark.parametrize("name", list(TRAIN_CONFS))
def test_train_cal_loss_fp16x3_against_fp64(name):
    """(l)"""
    conf = TRAIN_CONFS[name]
    batch = _batch()
    m = _model("fp16x3")
    loss, parts = TR.train_cal_loss(m, batch, conf)
    pix = "pixel_loss" if name == "l1" else "mse_loss"
    assert set(parts) == {"total_loss", pix, "degradation_loss"} | ({"ssim"} if name == "ssim" else set())
    m.zero_grad()
    loss.backward()
    r = _model("fp16x3")
    LR, HR = TR._prep(batch, conf, "cuda")
    out = r(LR)
    loss64, q64 = _loss64(out, HR, LR, conf)
    r.zero_grad()
    loss64.backward()
    l64 = float(loss64.detach())
    assert abs(float(loss.detach()) - l64) <= 1e-5 * abs(l64), (float(loss.detach()), l64)
    assert abs(float(parts["degradation_loss"]) - float(q64.detach().mean())) <= 1e-5 * float(q64.detach().mean())
    want = {n: p.grad.detach().cpu().double() for n, p in r.named_parameters()}
    worst = _gradcheck.check_grads({n: p.grad for n, p in m.named_parameters()}, want, tol=2e-5)
    z = _model("fp16x3")                                            # the bar can see the term
    l0, _ = TR.train_cal_loss(z, batch, dict(conf, degradation_loss_weight=0))
    l0.backward()
    moved = max(_gradcheck.relerr(a.grad, b.grad) for a, b in zip(z.parameters(), r.parameters())
                if float(b.grad.abs().max()) >= 1e-6)
    assert moved > 1e-3, moved
    print(f"[degrade] train_cal_loss fp16x3 {name}: loss {float(loss.detach()):.6f} (degradation "
          f"{float(parts['degradation_loss']):.6f}), worst parameter gradient {worst[0]:.2e} ({worst[1]}); without the "
          f"term the gradients are {moved:.2e} away")


@pytest.mark.parametrize("name", list(TRAIN_CONFS))
def test_train_cal_loss_bf16_is_the_engine_backward_of_the_launch(name):
    """(m)"""
    conf = TRAIN_CONFS[name]
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
    l2, dy = Fh.sr_loss_fwd_bwd(out.detach().float(), HR, lam_s, rng, window, sigma, pixel_kind=kind, pixel_param=param,
                                fg_weight=fw, fg_threshold=thr, deg_weight=LAM, deg_z=LR[:, 2], deg_gamma=GAMMA, deg_gain=10.0)
    r.zero_grad()
    out.backward(dy.to(out.dtype))
    assert torch.equal(loss.detach(), l2[0])
    for (n, a), (_, b) in zip(m.named_parameters(), r.named_parameters()):
        assert torch.equal(bits(a.grad), bits(b.grad)), n


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_weight_zero_is_the_step_without_the_key(impl):
    """(n)"""
    batch = _batch()
    for base in (TR.default_config(), dict(TR.default_config(), ssim_loss_weight=0.1, ssim_data_range=10.0)):
        a, b = _model(impl), _model(impl)
        la, pa = TR.train_cal_loss(a, batch, base)
        lb, pb = TR.train_cal_loss(b, batch + (torch.full((4,), 0.7).cuda(),),
                                   dict(base, degradation_loss_weight=0.0, degradation_gamma=0.7, degradation_channel=1))
        assert set(pa) == set(pb) and "degradation_loss" not in pb
        la.backward()
        lb.backward()
        assert torch.equal(la, lb)
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(bits(p.grad), bits(q.grad)), n


def test_three_tuple_batch():
    """(o)"""
    batch = _batch()
    a, b, c = _model("fp16x3"), _model("fp16x3"), _model("fp16x3")
    la, pa = TR.train_cal_loss(a, batch, DEG)
    g32 = torch.full((4,), GAMMA, dtype=torch.float32)
    conf_b = dict(DEG, degradation_gamma=float(g32[0]))             # the scalar the fp32 tensor holds
    lb0, _ = TR.train_cal_loss(c, batch, conf_b)
    lb, pb = TR.train_cal_loss(b, batch + (g32.cuda(),), dict(DEG, degradation_gamma=50.0))     # the batch's gamma overrides
    assert torch.equal(lb, lb0) and set(pa) == set(pb)
    assert abs(float(la) - float(lb)) <= 1e-6 * float(la)           # 0.7 and its fp32 rounding
    lb.backward()
    lb0.backward()
    for (n, p), (_, q) in zip(b.named_parameters(), c.named_parameters()):
        assert torch.equal(bits(p.grad), bits(q.grad)), n
    no_key = {k: v for k, v in DEG.items() if k != "degradation_gamma"}
    ld, _ = TR.train_cal_loss(_model("fp16x3"), batch + (g32.cuda(),), no_key)
    assert torch.equal(ld, lb)
    per = torch.tensor([0.05, 0.7, 5.0, 50.0])                      # and a varying one is the per-sample operator
    m = _model("fp16x3")
    lp, pp = TR.train_cal_loss(m, batch + (per,), no_key)            # a CPU gamma is moved with the batch
    LR, HR = TR._prep(batch, DEG, "cuda")
    with torch.no_grad():
        q64 = DC.restatement(_model("fp16x3")(LR).double().cpu(), LR[:, 2].double().cpu().reshape(4, 16), per.double(), 10.0)[1]
    assert abs(float(pp["degradation_loss"]) - float(q64.mean())) <= 1e-5 * float(q64.mean())
    with pytest.raises(_lib.TactileSRHipError):
        TR.train_cal_loss(m, batch, no_key)


def _same_state(ma, oa, mb, ob):
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]), n
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    for (n, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("form", ["scalar", "three_tuple"])
def test_graphed_step(form):
    """(p)"""
    conf = dict(DEG, ssim_loss_weight=0.1, ssim_data_range=10.0)
    batches = [_batch(seed=20 + i) for i in range(6)]
    if form == "three_tuple":
        conf.pop("degradation_gamma")
        gen = torch.Generator().manual_seed(77)
        batches = [b + ((0.05 * 1000 ** torch.rand(4, generator=gen)).cuda(),) for b in batches]
    me, mg = _model("fp16x3"), _model("fp16x3")
    oe = optim.Adam(me.parameters(), lr=1e-3, weight_decay=1e-2)
    og = optim.Adam(mg.parameters(), lr=1e-3, weight_decay=1e-2)
    gconf = copy.deepcopy(conf)
    gstep = GraphedTrainStep(mg, og, gconf, warmup=1)
    for i, b in enumerate(batches[:4]):                             # one eager warm-up step, then three replays
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert set(pe) == set(pg) == {"total_loss", "mse_loss", "ssim", "degradation_loss"}
        for k in pe:
            assert torch.equal(pe[k].detach(), pg[k]), (i, k, float(pe[k]), float(pg[k]))
    assert gstep.captures == 1
    _same_state(me, oe, mg, og)
    if form == "scalar":
        conf["degradation_gamma"] = gconf["degradation_gamma"] = 5.0    # a baked constant: dropped and recaptured
    else:
        conf["degradation_loss_weight"] = gconf["degradation_loss_weight"] = 0.25
        with pytest.raises(_lib.TactileSRHipError):                 # the signature holds the gamma's shape
            gstep(batches[4][:2])
    for i, b in enumerate(batches[4:]):
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert torch.equal(pe["total_loss"].detach(), pg["total_loss"]), i
        assert torch.equal(pe["degradation_loss"].detach(), pg["degradation_loss"]), i
    assert gstep.captures == 2
    _same_state(me, oe, mg, og)


def test_eval_func_degradation_score():
    """(q)"""
    m = _model("fp16x3")
    conf = dict(TR.default_config(), degradation_gamma=GAMMA)
    for loader in ([_batch(8, seed=31), _batch(8, seed=32)], [_batch(3, seed=33), _batch(3, seed=34), _batch(3, seed=35)]):
        three = TR.eval_func(m, loader, conf)
        four = TR.eval_func(m, loader, conf, degradation=True)
        five = TR.eval_func(m, loader, conf, windowed_ssim=True, degradation=True)
        assert len(three) == 3 and len(four) == 4 and len(five) == 5
        assert tuple(four[:3]) == tuple(three) and five[4] == four[3] and tuple(five[:3]) == tuple(three)
        want = 0.0
        with torch.no_grad():
            for b in loader:
                LR, HR = TR._prep(b, conf, "cuda")
                want += float(DC.restatement(m(LR).double().cpu(), LR[:, 2].double().cpu().reshape(-1, 16), GAMMA, 10.0)[1].mean())
        assert abs(four[3] - want / len(loader)) <= 1e-5 * want / len(loader), (four[3], want / len(loader))
    m.train()


def test_loader_yields_gamma_with_the_index():
    """(r)"""
    g = torch.Generator().manual_seed(9)
    n = 21
    LR, HR = torch.rand(n, 3, 4, 4, generator=g) * 8, SC.blobs(n, 100, 100, g)[:, 0] * 10
    gam = torch.arange(n, dtype=torch.float32) * 0.25 + 0.5
    ld = DeviceSRLoader(LR, HR, 4, shuffle=True, seed=3, device="cuda", augment="dihedral", taxel_noise=dict(sigma_add=0.02),
                        gamma=gam)
    seen = []
    for lr, hr, gm in ld:
        assert gm.is_cuda and gm.dtype == torch.float32 and torch.equal(gm.cpu(), gam[ld.last_index.cpu()])
        assert lr.shape[0] == hr.shape[0] == gm.shape[0]
        seen += ld.last_index.tolist()
    assert sorted(seen) == list(range(n))
    plain = DeviceSRLoader(LR, HR, 4, shuffle=True, seed=3, device="cuda", gamma=gam)
    m = _model("fp16x3")
    conf = {k: v for k, v in DEG.items() if k != "degradation_gamma"}
    for batch in plain:                                             # and the step takes the batch as it comes
        assert torch.equal(batch[2].cpu(), gam[plain.last_index.cpu()])
        loss, parts = TR.train_cal_loss(m, (batch[0], batch[1].unsqueeze(1), batch[2]), conf)
        assert math.isfinite(float(loss)) and "degradation_loss" in parts
        break
