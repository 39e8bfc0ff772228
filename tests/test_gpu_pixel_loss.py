"""GPU checks of the pixel losses (tsr_pixel_loss_fwd_bwd, functional.pixel_loss / pixel_loss_fwd_bwd / sr_loss_fwd_bwd, the
pixel keys of train_cal_loss and GraphedTrainStep) against the fp64 restatement and the bar of tests/_pixel_loss_cases.py.
Every output buffer is prefilled with NaN between NaN guard bands, and every launch runs twice and must give the same
bits."""
import copy
import math

import pytest
import torch

import _gradcheck
import _pixel_loss_cases as PC
import _ssim_cases as SC
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib, optim
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
INF = float("inf")


def _placed(n, off=0, fill=None):
    """n floats starting `off` floats past a 16-byte boundary, inside a NaN-filled device buffer with at least GUARD NaNs
    on either side: (buffer, the view, its start in the buffer)."""
    buf = torch.full((n + 2 * GUARD + 4,), NAN, dtype=torch.float32, device="cuda")
    start = GUARD + off
    mid = buf[start:start + n]
    assert mid.data_ptr() % 16 == 4 * off
    if fill is not None:
        mid.copy_(fill.reshape(-1))
    return buf, mid, start


def _guards_intact(buf, start, n):
    return bool(torch.isnan(buf[:start]).all() and torch.isnan(buf[start + n:]).all())


def _bits(x):
    return x.contiguous().view(torch.int32)


def _launch_once(y, t, a, want_dy, want_dt, prior, offs):
    n = y.numel()
    _, yd, _ = _placed(n, offs[0], y.cuda())
    _, td, _ = _placed(n, offs[1], t.cuda())
    lbuf, loss, ls = _placed(1)
    dbuf, dy, ds = _placed(n, offs[2], prior) if want_dy else (None, None, 0)
    tbuf, dt, ts = _placed(n, offs[3]) if want_dt else (None, None, 0)
    wbuf = torch.full((PC.WORK + 2 * GUARD,), NAN, dtype=torch.float64, device="cuda")
    work = wbuf[GUARD:GUARD + PC.WORK]
    args = dict(n=n, kind=PC.KIND_CODES[a["kind"]], param=a["param"] or 0.0, fg_weight=a["fg_weight"],
                fg_threshold=a["fg_threshold"], dy_scale=a.get("dy_scale", 1.0), accumulate=a.get("accumulate", 0))
    st = PC.call_raw(_lib.load(), args, y=yd.data_ptr(), t=td.data_ptr(), loss=loss.data_ptr(),
                     dy=dy.data_ptr() if want_dy else 0, dt=dt.data_ptr() if want_dt else 0, work=work.data_ptr(),
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, st
    assert _guards_intact(lbuf, ls, 1), "loss guard band written"
    assert bool(torch.isnan(wbuf[:GUARD]).all() and torch.isnan(wbuf[GUARD + PC.WORK:]).all()), "work guard band written"
    if want_dy:
        assert _guards_intact(dbuf, ds, n), "dy guard band written"
    if want_dt:
        assert _guards_intact(tbuf, ts, n), "dt guard band written"
    return (loss.clone().cpu(), dy.clone().cpu().view(y.shape) if want_dy else None,
            dt.clone().cpu().view(y.shape) if want_dt else None)


def launch(ref, want_dy=True, want_dt=False, dy_scale=1.0, accumulate=0, prior=None, offs=(0, 0, 0, 0), y=None, t=None):
    """Two launches on the reference's inputs (or the given y / t); the same bits required; CPU results."""
    y = ref["y"] if y is None else y
    t = ref["t"] if t is None else t
    a = dict(ref, dy_scale=dy_scale, accumulate=accumulate)
    pr = prior.cuda() if prior is not None else None
    r1 = _launch_once(y, t, a, want_dy, want_dt, pr, offs)
    r2 = _launch_once(y, t, a, want_dy, want_dt, pr, offs)
    for name, u, v in zip(("loss", "dy", "dt"), r1, r2):
        assert (u is None and v is None) or torch.equal(_bits(u), _bits(v)), f"two launches gave different {name} bits"
    return r1


WORST = {k: PC.Worst() for k in ("sizes", "big", "align", "dy", "dt")}


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", list(PC.SIZES))
def test_sizes(name):
    for kind, param, w, thr in PC.PARAMS:
        ref = PC.reference(name, kind, param, w, thr)
        loss, dy, dt = launch(ref, want_dt=True)
        PC.check(ref, loss, dy, dt, WORST["sizes"], label=(name, kind, param, w, thr))
    print(WORST["sizes"].line(f"sizes, up to {name}"))


@pytest.mark.parametrize("kind,param,w,thr", [("mse", None, 0.0, 0.0), ("huber", 0.25, 4.0, 0.5)])
def test_three_strides_of_the_capped_grid(kind, param, w, thr):
    """Every workgroup of the capped grid walks three strides, part of them a fourth, and three elements are left over;
    the data of every stride is scaled by its own factor."""
    ref = PC.reference(PC.BIG, kind, param, w, thr)
    loss, dy, dt = launch(ref, want_dt=True)
    PC.check(ref, loss, dy, dt, WORST["big"], label=(PC.BIG, kind))
    print(WORST["big"].line(f"{PC.BIG_N} elements, {kind}"))


_PTRS = ("y", "t", "dy", "dt")
ALIGN_CASES = ([(f"{p}+{o}", tuple(o if q == p else 0 for q in _PTRS)) for p in _PTRS for o in (1, 2, 3)] +
               [(f"all+{o}", (o, o, o, o)) for o in (1, 2, 3)] + [("mixed", (1, 2, 3, 0)), ("pairs", (2, 2, 1, 1))])


@pytest.mark.parametrize("label,offs", ALIGN_CASES, ids=[c[0] for c in ALIGN_CASES])
def test_alignment(label, offs):
    """y, t, dy, dt (offs in that order) moved 1, 2, 3 floats off 16-byte alignment: one at a time (no common offset:
    the float-at-a-time loop), all together (the float4 body behind a scalar head), and mixed."""
    for kind, param, w, thr in (("l1", None, 4.0, 0.5), ("charbonnier", 1e-3, 4.0, 0.0), ("huber", 0.25, 0.0, 0.0)):
        ref = PC.reference("align", kind, param, w, thr)
        loss, dy, dt = launch(ref, want_dt=True, offs=offs)
        PC.check(ref, loss, dy, dt, WORST["align"], label=(label, kind))
        l0, d0, t0 = launch(ref, want_dt=True)                     # a gradient element does not depend on the path
        assert torch.equal(_bits(dy), _bits(d0)) and torch.equal(_bits(dt), _bits(t0)), (label, kind)
        loss, dy, _ = launch(ref, offs=offs, accumulate=1, dy_scale=-0.25, prior=torch.ones(ref["y"].shape) * ref["scale"])
        PC.check(ref, loss, dy, None, WORST["align"], dy_scale=-0.25, prior=torch.ones(ref["y"].shape) * ref["scale"],
                 label=(label, kind, "accumulate"))
    print(WORST["align"].line(f"alignment, up to {label}"))


@pytest.mark.parametrize("kind,param", PC.KINDS)
def test_dy_contract(kind, param):
    ref = PC.reference("b2_40", kind, param, 4.0, 0.5)
    l_dy, g, _ = launch(ref)
    l_only, none, _ = launch(ref, want_dy=False)                   # dy = NULL: the value only, the same bits
    assert none is None and torch.equal(_bits(l_only), _bits(l_dy))
    gen = torch.Generator().manual_seed(5)
    prior = torch.randn(ref["y"].shape, generator=gen) * ref["scale"]
    for s in (1.0, -0.25, 0.0):
        loss, d, _ = launch(ref, dy_scale=s)                       # accumulate = 0 overwrites the NaN prefill
        assert torch.equal(_bits(loss), _bits(l_dy))
        PC.check(ref, loss, d, None, WORST["dy"], dy_scale=s, label=(kind, "overwrite", s))
        if s == 0:
            assert (d == 0).all()
        loss, d, _ = launch(ref, dy_scale=s, accumulate=1, prior=prior)
        assert torch.equal(_bits(loss), _bits(l_dy))
        PC.check(ref, loss, d, None, WORST["dy"], dy_scale=s, prior=prior, label=(kind, "accumulate", s))
        if s == 0:
            assert torch.equal(_bits(d), _bits(prior))
    print(WORST["dy"].line(f"dy contract, {kind} {param}"))


@pytest.mark.parametrize("kind,param,w,thr", PC.PARAMS)
def test_dt_contract(kind, param, w, thr):
    ref = PC.reference("k3r3", kind, param, w, thr)
    for s in (1.0, -0.25):
        loss, dy, dt = launch(ref, want_dt=True, dy_scale=s)
        assert torch.equal(_bits(dt), _bits(-dy)), (kind, s, "dt != -dy")
        PC.check(ref, loss, dy, dt, WORST["dt"], dy_scale=s, label=(kind, "dt", s))
        l2, none, dt2 = launch(ref, want_dy=False, want_dt=True, dy_scale=s)         # dt alone
        assert none is None and torch.equal(_bits(l2), _bits(loss)) and torch.equal(_bits(dt2), _bits(dt))
        prior = torch.full(ref["y"].shape, 3.0) * ref["scale"]
        _, _, dt3 = launch(ref, want_dt=True, dy_scale=s, accumulate=1, prior=prior)  # dt is overwritten, never accumulated
        assert torch.equal(_bits(dt3), _bits(dt))


@pytest.mark.parametrize("kind,param", PC.KINDS)
def test_non_finite_inputs_stay_in_their_own_element(kind, param):
    ref = PC.reference("b2_40", kind, param, 4.0, 0.5)
    s = -0.25
    _, d0, t0 = launch(ref, want_dt=True, dy_scale=s)
    y, t = ref["y"].clone().flatten(), ref["t"].clone().flatten()
    contact = [int(i) for i in torch.nonzero(t > 0.5).flatten()[:2]]
    back = [int(i) for i in torch.nonzero(t == 0).flatten()[:2]]
    i_nan, i_tnan = contact[0], back[0]
    delta = {"l1": 1.0, "huber": param}.get(kind)
    for i_inf, is_contact in ((contact[1], True), (back[1], False)):
        yy = y.clone()
        yy[i_inf] = INF
        loss, d1, t1 = launch(ref, want_dt=True, dy_scale=s, y=yy.view(ref["y"].shape))
        assert float(loss) == INF                                  # no NaN: +Inf
        if kind == "mse":
            want = -INF                                            # dy_scale < 0
        elif kind == "charbonnier":
            want = NAN                                             # Inf / Inf
        else:
            want = delta * PC.coefficient(ref, s, is_contact)
        for got, sign in ((d1.flatten()[i_inf], 1.0), (t1.flatten()[i_inf], -1.0)):
            assert (math.isnan(float(got)) if math.isnan(want) else float(got) == sign * want), (kind, float(got), want)
        keep = torch.ones(y.numel(), dtype=torch.bool)
        keep[i_inf] = False
        assert torch.equal(_bits(d1.flatten()[keep]), _bits(d0.flatten()[keep]))
        assert torch.equal(_bits(t1.flatten()[keep]), _bits(t0.flatten()[keep]))
        yy[i_nan] = NAN
        tt = t.clone()
        tt[i_tnan] = NAN
        loss, d2, t2 = launch(ref, want_dt=True, dy_scale=s, y=yy.view(ref["y"].shape), t=tt.view(ref["y"].shape))
        assert math.isnan(float(loss))
        for i in (i_nan, i_tnan):
            assert math.isnan(float(d2.flatten()[i])) and math.isnan(float(t2.flatten()[i])), (kind, i)
        assert torch.equal(_bits(d2.flatten()[i_inf]), _bits(d1.flatten()[i_inf]))
        keep[i_nan] = keep[i_tnan] = False
        assert torch.equal(_bits(d2.flatten()[keep]), _bits(d0.flatten()[keep]))
        assert torch.equal(_bits(t2.flatten()[keep]), _bits(t0.flatten()[keep]))


def _refusal_call(a):
    n = 100
    y = torch.rand(n, device="cuda")
    bufs = {k: _placed(n if k in ("dy", "dt") else 1) for k in ("loss", "dy", "dt")}
    work = torch.full((PC.WORK,), NAN, dtype=torch.float64, device="cuda")
    addr = dict(y=y.data_ptr(), t=y.data_ptr(), work=work.data_ptr(), **{k: v[1].data_ptr() for k, v in bufs.items()})
    ptrs = {k: (addr["dy"] if a[k] == "dy" else (addr[k] if a[k] else 0)) for k in addr}
    st = PC.call_raw(_lib.load(), a, stream=torch.cuda.current_stream().cuda_stream, **ptrs)
    torch.cuda.synchronize()
    return st, bufs, work


@pytest.mark.parametrize("label,over", PC.REFUSALS, ids=[r[0] for r in PC.REFUSALS])
def test_refusal_matrix(label, over):
    st, bufs, work = _refusal_call(dict(PC.BASE_ARGS, **over))
    assert st == 1, (label, st)
    assert all(torch.isnan(b[0]).all() for b in bufs.values()) and torch.isnan(work).all(), (label, "a refused call wrote")


@pytest.mark.parametrize("label,over", PC.ACCEPTED, ids=[r[0] for r in PC.ACCEPTED])
def test_the_table_refuses_no_more_than_the_header(label, over):
    a = dict(PC.BASE_ARGS, **over)
    st, bufs, _ = _refusal_call(a)
    assert st == 0, (label, st)
    assert torch.isfinite(bufs["loss"][1]).all()
    for k in ("dy", "dt"):
        assert bool(torch.isfinite(bufs[k][1]).all()) == bool(a[k]) and _guards_intact(bufs[k][0], bufs[k][2], 100), (label, k)


# ------------------------------------------------------------------------------------------ functional layer
@pytest.mark.parametrize("kind,param", [("l1", None), ("charbonnier", None), ("huber", 0.25)])
def test_pixel_loss_backward_to_prediction_and_target(kind, param):
    p = PC.KINDS[2][1] if (kind, param) == ("charbonnier", None) else param       # param=None: the default eps
    ref = PC.reference("b2_40", kind, p, 4.0, 0.5)
    y = ref["y"].cuda().requires_grad_(True)
    t = ref["t"].cuda().requires_grad_(True)
    loss = Fh.pixel_loss(y, t, kind, param, 4.0, 0.5)
    (0.37 * loss).backward()
    PC.check(ref, loss.detach().cpu().view(1), y.grad.cpu(), t.grad.cpu(), dy_scale=0.37, label=("pixel_loss", kind),
             exact=False)                                          # autograd multiplies by 0.37 in fp32: a second rounding
    assert torch.equal(_bits(t.grad), _bits(-y.grad))
    y2 = ref["y"].cuda().requires_grad_(True)                      # a target that asks for none gets none
    t2 = ref["t"].cuda()
    l2 = Fh.pixel_loss(y2, t2, kind, param, 4.0, 0.5)
    (0.37 * l2).backward()
    assert t2.grad is None and torch.equal(l2.detach(), loss.detach()) and torch.equal(y2.grad, y.grad)


def test_pixel_loss_fwd_bwd_arguments():
    ref = PC.reference("b2_40", "huber", 1.0, 4.0, 0.5)
    y, t = ref["y"].cuda(), ref["t"].cuda()
    loss, dy = Fh.pixel_loss_fwd_bwd(y, t, "huber", None, 4.0, 0.5)            # delta defaults to 1.0
    PC.check(ref, loss.cpu(), dy.cpu(), label="fwd_bwd")
    prior = torch.full_like(y, 2.0) * ref["scale"]
    given = prior.clone()
    l2, d2, dt = Fh.pixel_loss_fwd_bwd(y, t, "HUBER", 1.0, 4.0, 0.5, dy=given, dy_scale=-0.25, accumulate=True, want_dt=True)
    assert d2 is given and torch.equal(l2, loss)
    PC.check(ref, l2.cpu(), d2.cpu(), dt.cpu(), dy_scale=-0.25, prior=prior.cpu(), label="fwd_bwd accumulate")
    for bad in (dict(kind="l2"), dict(kind="huber", param=0.0), dict(fg_weight=-1.0), dict(fg_threshold=NAN),
                dict(accumulate=True), dict(dy=torch.empty(3, device="cuda")), dict(dy_scale=NAN)):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.pixel_loss_fwd_bwd(y, t, **bad)
    with pytest.raises(_lib.TactileSRHipError):
        Fh.pixel_loss_fwd_bwd(y, t[:1])


def test_sr_loss_fwd_bwd_with_a_pixel_kind_and_an_ssim_term():
    sref = SC.reference("w11_5x40x40", "clamped")
    y, t = sref["y"].cuda(), sref["t"].cuda()
    B, lam = y.shape[0], 0.1
    l0, d0 = Fh.sr_loss_fwd_bwd(y, t, 0.0, pixel_kind="mse", fg_weight=0.0, fg_threshold=0.3)      # today's launch
    lm, dm = Fh.mse_fwd_bwd(y, t)
    assert torch.equal(l0, lm) and torch.equal(d0, dm)
    pref = PC.build_reference(sref["y"], sref["t"], "huber", 0.25, 4.0, 0.5)
    lp, dp = Fh.sr_loss_fwd_bwd(y, t, 0.0, pixel_kind="huber", pixel_param=0.25, fg_weight=4.0, fg_threshold=0.5)
    l1, d1 = Fh.pixel_loss_fwd_bwd(y, t, "huber", 0.25, 4.0, 0.5)
    assert torch.equal(lp, l1) and torch.equal(dp, d1)
    PC.check(pref, lp.cpu(), dp.cpu(), label="sr_loss_fwd_bwd, no ssim term")
    loss, dy, pix, vals = Fh.sr_loss_fwd_bwd(y, t, lam, pixel_kind="huber", pixel_param=0.25, fg_weight=4.0,
                                             fg_threshold=0.5, return_parts=True)
    assert torch.equal(pix, lp)
    want = pref["l64"] + lam * (1 - float(sref["v64"].mean()))
    assert abs(float(loss) - want) <= PC.BAR * want, (float(loss), want)
    g64 = pref["g64"] - lam / B * sref["g64"]
    err = float((dy.cpu().double() - g64).abs().max() / g64.abs().max())
    assert err <= PC.BAR, err
    moved = float((dy.cpu().double() - pref["g64"]).abs().max() / g64.abs().max())
    assert moved > 100 * PC.BAR, moved                             # the bar can see the SSIM term in the sum


# ------------------------------------------------------------------------------------------ train step
def _model(impl, seed=42):
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR(10, 1, 3, 1, 1).cuda().train()
    m.train_impl = impl
    return m


def _batch(B=4, seed=11):
    """Random taxels and a contact-like HR: blobs of amplitude <= 100 raw, <= 10 after HR_scale_num."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (SC.blobs(B, 100, 100, g) * 10).cuda()


PIX_CONF = dict(TR.default_config(), contact_loss_weight=4.0, contact_threshold=0.5)
TRAIN_KINDS = [("l1", None), ("charbonnier", None), ("huber", 0.5)]


@pytest.mark.parametrize("kind,param", TRAIN_KINDS)
def test_train_cal_loss_fp16x3_against_fp64(kind, param):
    conf = dict(PIX_CONF, pixel_loss=kind, pixel_loss_param=param)
    name, p, w, thr = TR.pixel_loss_config(conf)
    batch = _batch()
    m = _model("fp16x3")
    loss, parts = TR.train_cal_loss(m, batch, conf)
    assert set(parts) == {"total_loss", "pixel_loss"} and torch.equal(parts["pixel_loss"].detach(), loss.detach())
    m.zero_grad()
    loss.backward()
    # the same model driven through autograd by the fp64 restatement on ITS OWN output (the device's ReLU pattern); where
    # the fp64 gradient rounds to the launch's own fp32 dy the two backward passes see one input and the error is 0
    r = _model("fp16x3")
    LR, HR = TR._prep(batch, conf, "cuda")
    out = r(LR)
    assert 0.01 < float((HR > thr).float().mean()) < 0.9           # the weight splits the pixels
    loss64 = PC.restatement(out.double().cpu(), HR.double().cpu(), name, p, w, thr)      # fp64 on the host; autograd crosses
    r.zero_grad()
    loss64.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-5 * abs(float(loss64.detach())), (float(loss.detach()), float(loss64.detach()))
    want = {n: q.grad.detach().cpu().double() for n, q in r.named_parameters()}
    worst = _gradcheck.check_grads({n: q.grad for n, q in m.named_parameters()}, want, tol=2e-5)
    # the bar can see the criterion: today's loss on the same model gives gradients far outside it
    z = _model("fp16x3")
    l0, _ = TR.train_cal_loss(z, batch, TR.default_config())
    l0.backward()
    moved = max(_gradcheck.relerr(a.grad, b.grad) for a, b in zip(z.parameters(), r.parameters())
                if float(b.grad.abs().max()) >= 1e-6)
    assert moved > 1e-3, moved
    print(f"[pixel loss] train_cal_loss fp16x3 {kind}: loss {float(loss.detach()):.6f}, worst parameter gradient "
          f"{worst[0]:.2e} ({worst[1]}); the MSE gradients are {moved:.2e} away")


@pytest.mark.parametrize("kind,param", TRAIN_KINDS)
def test_train_cal_loss_bf16_is_the_engine_backward_of_the_launch(kind, param):
    conf = dict(PIX_CONF, pixel_loss=kind, pixel_loss_param=param)
    batch = _batch()
    m = _model("bf16")
    loss, parts = TR.train_cal_loss(m, batch, conf)
    assert set(parts) == {"total_loss", "pixel_loss"}
    m.zero_grad()
    loss.backward()
    r = _model("bf16")
    LR, HR = TR._prep(batch, conf, "cuda")
    out = r(LR)
    l2, dy = Fh.pixel_loss_fwd_bwd(out.detach().float(), HR, *TR.pixel_loss_config(conf))
    r.zero_grad()
    out.backward(dy.to(out.dtype))
    assert torch.equal(loss.detach(), l2[0])
    ref = PC.build_reference(out.detach().float().cpu(), HR.cpu(), *TR.pixel_loss_config(conf))
    PC.check(ref, l2.cpu(), dy.cpu(), label=("bf16 launch", kind))                 # and the launch's dy is the criterion's
    for (n, a), (_, b) in zip(m.named_parameters(), r.named_parameters()):
        assert torch.equal(_bits(a.grad), _bits(b.grad)), n


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_default_keys_are_todays_step_bit_for_bit(impl):
    batch = _batch()
    a, b, c = _model(impl), _model(impl), _model(impl)
    la, pa = TR.train_cal_loss(a, batch, TR.default_config())
    lb, pb = TR.train_cal_loss(b, batch, dict(TR.default_config(), pixel_loss="mse", contact_loss_weight=0,
                                               pixel_loss_param=0.5, contact_threshold=0.3))
    LR, HR = TR._prep(batch, TR.default_config(), "cuda")
    lc = Fh.mse_loss(c(LR), HR)                                    # the step as it was: the MSE launch through autograd
    assert set(pa) == set(pb) == {"total_loss"}
    for loss in (la, lb, lc):
        loss.backward()
    assert torch.equal(la, lc) and torch.equal(lb, lc)
    for (n, p), (_, q), (_, s) in zip(a.named_parameters(), b.named_parameters(), c.named_parameters()):
        assert torch.equal(_bits(p.grad), _bits(s.grad)) and torch.equal(_bits(q.grad), _bits(s.grad)), n


def test_pixel_and_ssim_keys_together():
    conf = dict(PIX_CONF, pixel_loss="huber", ssim_loss_weight=0.1, ssim_data_range=10.0)
    m = _model("fp16x3")
    loss, parts = TR.train_cal_loss(m, _batch(), conf)
    assert set(parts) == {"total_loss", "pixel_loss", "ssim"}
    want = float(parts["pixel_loss"]) + 0.1 * (1 - float(parts["ssim"]))
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want)
    _, parts = TR.train_cal_loss(m, _batch(), dict(TR.default_config(), ssim_loss_weight=0.1, ssim_data_range=10.0))
    assert set(parts) == {"total_loss", "mse_loss", "ssim"}         # the plain MSE keeps its name
    with pytest.raises(_lib.TactileSRHipError):
        TR.train_cal_loss(m, _batch(), dict(conf, pixel_loss="l2"))


def _same_state(ma, oa, mb, ob):
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]), n
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    for (n, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(a, b), n


def test_graphed_step_with_a_pixel_criterion():
    conf = dict(PIX_CONF, pixel_loss="charbonnier")
    batches = [_batch(seed=20 + i) for i in range(6)]
    me, mg = _model("fp16x3"), _model("fp16x3")
    oe = optim.Adam(me.parameters(), lr=1e-3, weight_decay=1e-2)
    og = optim.Adam(mg.parameters(), lr=1e-3, weight_decay=1e-2)
    gconf = copy.deepcopy(conf)
    gstep = GraphedTrainStep(mg, og, gconf, warmup=1)
    for i, b in enumerate(batches[:4]):                             # one eager warm-up step, then three replays
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert set(pe) == set(pg) == {"total_loss", "pixel_loss"}
        for k in pe:
            assert torch.equal(pe[k].detach(), pg[k]), (i, k, float(pe[k]), float(pg[k]))
    assert gstep.captures == 1
    _same_state(me, oe, mg, og)
    conf["pixel_loss_param"] = gconf["pixel_loss_param"] = 0.05     # a baked constant: the graph is dropped and recaptured
    for i, b in enumerate(batches[4:]):
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert torch.equal(pe["total_loss"].detach(), pg["total_loss"]), i
    assert gstep.captures == 2
    _same_state(me, oe, mg, og)
