"""GPU checks of the differentiable SSIM (tsr_ssim_fwd_bwd, functional.ssim / ssim_loss / sr_loss_fwd_bwd, the SSIM term
of train_cal_loss and GraphedTrainStep, eval_func's windowed average) against the fp64 restatement and the rule of
tests/_ssim_cases.py.  Every output buffer is prefilled with NaN between NaN guard bands, and every launch runs twice and
must give the same bits."""
import copy

import pytest
import torch

import _gradcheck
import _ssim_cases as SC
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib, optim
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")


def _guarded(n, fill=None):
    """A NaN-filled device buffer of n + 2 GUARD floats; the middle n (a view) optionally set to `fill`."""
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device="cuda")
    mid = buf[GUARD:GUARD + n]
    if fill is not None:
        mid.copy_(fill.reshape(-1))
    return buf, mid


def _guards_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all())


def _bits(x):
    return x.contiguous().view(torch.int32)


def _launch_once(y, t, a, want_dy, prior):
    B, _, H, W = y.shape
    vbuf, vals = _guarded(B)
    dbuf, dy = _guarded(y.numel(), prior) if want_dy else (None, None)
    args = dict(B=B, H=H, W=W, win=a["win"], sigma=a["sigma"], C1=a["C1"], C2=a["C2"], dy_scale=a.get("dy_scale", 1.0),
                accumulate=a.get("accumulate", 0))
    st = SC.call_raw(_lib.load(), args, y=y.data_ptr(), t=t.data_ptr(), ssim=vals.data_ptr(),
                     dy=dy.data_ptr() if want_dy else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, st
    assert _guards_intact(vbuf, B), "ssim guard band written"
    if want_dy:
        assert _guards_intact(dbuf, y.numel()), "dy guard band written"
    return vals.clone(), (dy.clone().view_as(y) if want_dy else None)


def launch(ref, want_dy=True, dy_scale=1.0, accumulate=0, prior=None, y=None):
    """Two launches on the reference's inputs; the same bits required; CPU results."""
    y = (ref["y"] if y is None else y).cuda().contiguous()
    t = ref["t"].cuda().contiguous()
    a = dict(ref, dy_scale=dy_scale, accumulate=accumulate)
    v1, d1 = _launch_once(y, t, a, want_dy, prior)
    v2, d2 = _launch_once(y, t, a, want_dy, prior)
    assert torch.equal(_bits(v1), _bits(v2)), "two launches gave different ssim bits"
    if want_dy:
        assert torch.equal(_bits(d1), _bits(d2)), "two launches gave different dy bits"
    return v1.cpu(), (d1.cpu() if want_dy else None)


WORST = {"windowed": SC.Worst(), "global": SC.Worst(), "impulse": SC.Worst(), "walk": SC.Worst(), "dy": SC.Worst()}


@pytest.mark.parametrize("name", [c[0] for c in SC.WINDOW_CASES])
def test_windowed_cases(name):
    for law in SC.LAWS:
        ref = SC.reference(name, law)
        vals, dy = launch(ref)
        assert not torch.isnan(dy).any(), (name, law, "dy not fully written")
        SC.check(ref, vals, dy, WORST["windowed"], label=(name, law))
    print(WORST["windowed"].line(f"windowed, up to {name}"))


@pytest.mark.parametrize("name", [c[0] for c in SC.GLOBAL_CASES])
def test_global_cases(name):
    for law in SC.LAWS:
        ref = SC.reference(name, law)
        vals, dy = launch(ref)
        assert not torch.isnan(dy).any(), (name, law, "dy not fully written")
        SC.check(ref, vals, dy, WORST["global"], label=(name, law))
        _, ss = Fh.psnr_ssim(ref["y"].cuda(), ref["t"].cuda(), 250.0, C1=ref["C1"], C2=ref["C2"])
        assert (vals - ss.cpu()).abs().max() <= 1e-6, (name, law)
    print(WORST["global"].line(f"global, up to {name}"))


@pytest.mark.parametrize("H,W", SC.IMPULSE_SHAPES)
def test_impulses(H, W):
    ref = SC.impulse_reference(H, W)
    vals, dy = launch(ref)
    SC.check(ref, vals, dy, WORST["impulse"], label=("impulse", H, W))
    print(WORST["impulse"].line(f"impulses, up to {H}x{W}"))


@pytest.mark.parametrize("name", ["w11_3x13x29", "w11_5x40x40", "g_3x1x7", "g_4x40x40"])
def test_dy_contract(name):
    ref = SC.reference(name, "clamped")
    v_dy, g = launch(ref)
    v_only, none = launch(ref, want_dy=False)                   # dy = NULL: values only, the same bits
    assert none is None and torch.equal(_bits(v_only), _bits(v_dy))
    gen = torch.Generator().manual_seed(5)
    prior = torch.randn(ref["y"].shape, generator=gen) * ref["scale"].float().view(-1, 1, 1, 1)
    for s in (1.0, -0.25, 0.0):
        v, d = launch(ref, dy_scale=s)                          # accumulate = 0 overwrites the NaN prefill
        assert not torch.isnan(d).any() and torch.equal(_bits(v), _bits(v_dy))
        SC.check(ref, v, d, WORST["dy"], grad_factor=s, label=(name, "overwrite", s))
        v, d = launch(ref, dy_scale=s, accumulate=1, prior=prior.cuda())
        SC.check(ref, v, d, WORST["dy"], grad_factor=s, prior=prior, label=(name, "accumulate", s))
    print(WORST["dy"].line(f"dy contract, up to {name}"))


@pytest.mark.parametrize("win", [11, 0])
@pytest.mark.parametrize("poison", [NAN, float("inf")], ids=["nan", "inf"])
def test_isolation(win, poison):
    ref = SC.reference("w11_5x40x40" if win else "g_4x40x40", "clamped")
    ref = {k: (v[:4] if torch.is_tensor(v) else v) for k, v in ref.items()}
    v0, d0 = launch(ref)
    y = ref["y"].clone()
    y[1, 0, 17, 23] = poison
    v1, d1 = launch(ref, y=y)
    assert torch.isnan(v1[1])
    assert torch.isnan(d1[1, 0, 17, 23])
    if win == 0:
        assert torch.isnan(d1[1]).all()                         # one window holds every pixel
    else:                                                       # as in torch: NaN exactly where a window holds the pixel
        far = torch.ones(40, 40, dtype=torch.bool)
        far[17 - 10:17 + 11, 23 - 10:23 + 11] = False
        assert torch.isnan(d1[1, 0][~far]).all() and torch.equal(_bits(d1[1, 0][far]), _bits(d0[1, 0][far]))
    keep = [0, 2, 3]
    assert torch.equal(_bits(v1[keep]), _bits(v0[keep])) and torch.equal(_bits(d1[keep]), _bits(d0[keep]))


def test_batch_walk():
    ref = SC.walk_reference()
    vals, dy = launch(ref)
    SC.check(ref, vals, dy, WORST["walk"], label="walk")
    print(WORST["walk"].line("batch walk, 2100 images"))


@pytest.mark.parametrize("label,over", SC.REFUSALS, ids=[r[0] for r in SC.REFUSALS])
def test_refusal_matrix(label, over):
    a = dict(SC.BASE_ARGS, **over)
    n = 2 * 13 * 29                                             # the buffers of the base shape; a refusal reads none
    y = torch.rand(n, device="cuda")
    vbuf, vals = _guarded(2)
    dbuf, dy = _guarded(n)
    st = SC.call_raw(_lib.load(), a, y=y.data_ptr() if a["y"] else 0, t=y.data_ptr() if a["t"] else 0,
                     ssim=vals.data_ptr() if a["ssim"] else 0, dy=dy.data_ptr() if a["dy"] else 0,
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 1, (label, st)
    assert torch.isnan(vbuf).all() and torch.isnan(dbuf).all(), (label, "a refused call wrote")


def test_functional_refuses_through_the_status():
    a = torch.rand(2, 1, 13, 29, device="cuda")
    for kw in (dict(window=4), dict(window=13), dict(sigma=0.0), dict(data_range=0.0)):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.ssim(a, a, **kw)
    with pytest.raises(_lib.TactileSRHipError):
        Fh.ssim(a[:, :, :10], a[:, :, :10])


# ------------------------------------------------------------------------------------------ golden: the reference's own values
def test_global_form_matches_the_reference_code(golden):
    g = golden("ssim")
    y, t = torch.from_numpy(g["y"])[:, None].cuda(), torch.from_numpy(g["t"])[:, None].cuda()
    for i in range(2):                                          # B = 1, as the reference's functions take one pair
        want, f32 = float(g["calc_f64"][i]), float(g["calc_f32"][i])
        got = float(Fh.ssim(y[i:i + 1], t[i:i + 1], window=0)[0])
        assert abs(got - want) <= max(1e-5, min(4 * abs(f32 - want), SC.CAP)), (i, got, want, f32)
        assert abs(float(g["module_f64"][i]) - want) <= 1e-12
        yi = y[i:i + 1].clone().requires_grad_(True)
        loss = Fh.ssim_loss(yi, t[i:i + 1], window=0)
        loss.backward()
        assert abs(float(loss.detach()) - (1 - want)) <= max(1e-5, min(4 * abs(f32 - want), SC.CAP))
        gref = -torch.from_numpy(g["grad_f64"][i])              # d (1 - ssim) / d y
        err = float((yi.grad[0, 0].cpu().double() - gref).abs().max() / gref.abs().max())
        assert err <= 1e-5, (i, err)


# ------------------------------------------------------------------------------------------ module level
def test_ssim_loss_backward_with_an_upstream_gradient():
    ref = SC.reference("w11_5x40x40", "clamped")
    B = ref["y"].shape[0]
    y = ref["y"].cuda().requires_grad_(True)
    loss = Fh.ssim_loss(y, ref["t"].cuda())
    (3.0 * loss).backward()
    assert abs(float(loss.detach()) - (1 - float(ref["v64"].mean()))) <= 1e-5
    SC.check(ref, Fh.ssim(y.detach(), ref["t"].cuda()).cpu(), y.grad.cpu(), grad_factor=-3.0 / B, label="ssim_loss")
    with pytest.raises(_lib.TactileSRHipError):
        Fh.ssim_loss(ref["y"], ref["t"])


def test_sr_loss_fwd_bwd_is_the_two_launches():
    ref = SC.reference("w11_5x40x40", "clamped")
    y, t = ref["y"].cuda(), ref["t"].cuda()
    B, lam = y.shape[0], 0.1
    l0, d0 = Fh.sr_loss_fwd_bwd(y, t, 0.0)
    lm, dm = Fh.mse_fwd_bwd(y, t)
    assert torch.equal(l0, lm) and torch.equal(d0, dm)
    loss, dy = Fh.sr_loss_fwd_bwd(y, t, lam)
    mse64 = float(((ref["y"].double() - ref["t"].double()) ** 2).mean())
    want = mse64 + lam * (1 - float(ref["v64"].mean()))
    assert abs(float(loss) - want) <= 1e-5 * want
    g64 = 2 * (ref["y"].double() - ref["t"].double()) / y.numel() - lam / B * ref["g64"]
    err = (dy.cpu().double() - g64).abs().amax(dim=(1, 2, 3)) / g64.abs().amax(dim=(1, 2, 3))
    assert (err <= 1e-5).all(), err.tolist()


def _model(impl, seed=42):
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR(10, 1, 3, 1, 1).cuda().train()
    m.train_impl = impl
    return m


def _batch(B=4, seed=11):
    """Random taxels and a contact-like HR: blobs of amplitude <= 100 raw, <= 10 after HR_scale_num.  On white-noise
    targets the SSIM term's share of dy is ~1e-7 (nothing a gradient bar could see); here it is percents."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (SC.blobs(B, 100, 100, g) * 10).cuda()


CONF = dict(TR.default_config(), ssim_data_range=10.0)


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_train_cal_loss_with_an_ssim_term(impl):
    lam = 0.1
    conf = dict(CONF, ssim_loss_weight=lam)
    batch = _batch()
    m = _model(impl)
    loss, parts = TR.train_cal_loss(m, batch, conf)
    assert set(parts) == {"total_loss", "mse_loss", "ssim"}
    m.zero_grad()
    loss.backward()
    # the same model driven through autograd by the MSE launch plus the fp64 restatement on ITS OWN output
    r = _model(impl)
    LR, HR = TR._prep(batch, conf, "cuda")
    out = r(LR)
    C1, C2 = SC.constants(conf["ssim_data_range"])
    ssim64 = SC.restatement(out.double().cpu(), HR.double().cpu(), 11, 1.5, C1, C2)     # fp64 on the host; autograd crosses
    ref_loss = Fh.mse_loss(out, HR) + (lam * (1 - ssim64.mean())).cuda()
    r.zero_grad()
    ref_loss.backward()
    loss64 = float(((out.detach().double() - HR.double()) ** 2).mean() + lam * (1 - ssim64.detach().mean()))
    assert abs(float(loss.detach()) - loss64) <= 1e-5 * abs(loss64), (float(loss.detach()), loss64)
    assert abs(float(parts["ssim"]) - float(ssim64.detach().mean())) <= 1e-5
    assert abs(float(parts["mse_loss"]) + lam * (1 - float(parts["ssim"])) - float(loss.detach())) <= 1e-6 * abs(loss64)
    want = {n: p.grad.detach().cpu().double() for n, p in r.named_parameters()}
    worst = _gradcheck.check_grads({n: p.grad for n, p in m.named_parameters()}, want, tol=2e-5)
    # the bar can see the term: without it (today's loss on the same model) the gradients are far outside the bar
    z = _model(impl)
    l0, _ = TR.train_cal_loss(z, batch, TR.default_config())
    l0.backward()
    moved = max(_gradcheck.relerr(p.grad, q.grad) for p, q in zip(z.parameters(), r.parameters())
                if float(q.grad.abs().max()) >= 1e-6)
    assert moved > 1e-3, moved
    print(f"[ssim] train_cal_loss {impl}: loss {float(loss.detach()):.6f} (mse {float(parts['mse_loss']):.6f}, ssim "
          f"{float(parts['ssim']):.6f}), worst parameter gradient {worst[0]:.2e} ({worst[1]}); the MSE-only gradients "
          f"are {moved:.2e} away")


def test_zero_weight_is_todays_step_bit_for_bit():
    batch = _batch()
    a, b = _model("fp16x3"), _model("fp16x3")
    la, pa = TR.train_cal_loss(a, batch, TR.default_config())
    lb, pb = TR.train_cal_loss(b, batch, dict(CONF, ssim_loss_weight=0.0, ssim_window=7))
    assert set(pa) == set(pb) == {"total_loss"}
    la.backward()
    lb.backward()
    assert torch.equal(la, lb)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def _same_state(ma, oa, mb, ob):
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]), n
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    for (n, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(a, b), n


def test_graphed_step_with_an_ssim_term():
    conf = dict(CONF, ssim_loss_weight=0.1)
    batches = [_batch(seed=20 + i) for i in range(6)]
    me, mg = _model("fp16x3"), _model("fp16x3")
    oe = optim.Adam(me.parameters(), lr=1e-3, weight_decay=1e-2)
    og = optim.Adam(mg.parameters(), lr=1e-3, weight_decay=1e-2)
    gconf = copy.deepcopy(conf)
    gstep = GraphedTrainStep(mg, og, gconf, warmup=1)
    for i, b in enumerate(batches[:4]):                         # one eager warm-up step, then three replays
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert set(pe) == set(pg) == {"total_loss", "mse_loss", "ssim"}
        for k in pe:
            assert torch.equal(pe[k].detach(), pg[k]), (i, k, float(pe[k]), float(pg[k]))
    assert gstep.captures == 1
    _same_state(me, oe, mg, og)
    conf["ssim_loss_weight"] = gconf["ssim_loss_weight"] = 0.25  # a baked constant: the graph is dropped and recaptured
    for i, b in enumerate(batches[4:]):
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert torch.equal(pe["total_loss"].detach(), pg["total_loss"]), i
    assert gstep.captures == 2
    _same_state(me, oe, mg, og)


def test_eval_func_windowed_average():
    m = _model("fp16x3")
    conf = dict(CONF, ssim_window=7, ssim_sigma=1.0)
    loader = [_batch(seed=31), _batch(seed=32)]
    three = TR.eval_func(m, loader, conf)
    four = TR.eval_func(m, loader, conf, windowed_ssim=True)
    assert len(three) == 3 and len(four) == 4 and tuple(four[:3]) == tuple(three)
    want = 0.0
    C1, C2 = SC.constants(conf["ssim_data_range"])
    with torch.no_grad():
        for b in loader:
            LR, HR = TR._prep(b, conf, "cuda")
            want += float(SC.restatement(m(LR).double().cpu(), HR.double().cpu(), 7, 1.0, C1, C2).mean())
    assert abs(four[3] - want / 2) <= 1e-5, (four[3], want / 2)
