"""GPU checks of d loss / d taxels through the train step (``LR.requires_grad_()`` in train mode): the stem data-gradient
kernels against fp64 autograd of the reference's Upsample + Conv2d, and the whole network's ``LR.grad`` against the fp64
oracle evaluated on the device's own ReLU pattern (tests/_gradcheck.py explains why the pattern is forced)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd  # noqa: F401
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cosine(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("b16", [False, True])
@pytest.mark.parametrize("B,sf", [(1, 10), (3, 10), (130, 10), (2, 25)])
def test_stem_dgrad_kernel_vs_fp64_autograd(T, B, sf, b16):
    """dx of conv3x3(interpolate(x)) for a random CB16 cotangent dz, 64 channels at offset 64 of a 128-channel tensor,
    written into channels 3t .. 3t+2 of a 24-channel dx: stores for t = 0..7, then an accumulating launch on top."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(B * 31 + sf + int(b16))
    hin = win = 4
    H, W = hin * sf, win * sf
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
    dz = [torch.randn(B, 64, H, W, generator=g) for _ in range(9)]
    if b16:
        dz = [d.bfloat16().float() for d in dz]           # the oracle sees the same bf16-rounded cotangent
    dt = torch.bfloat16 if b16 else torch.float32
    name = "tsr_stem_dgrad_b16" if b16 else "tsr_stem_dgrad"

    def ref(d):
        x = torch.zeros(B, 3, hin, win, dtype=torch.float64, requires_grad=True)
        z = F.conv2d(F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False), w.double(), padding=1)
        (gx,) = torch.autograd.grad(z, x, d.double())
        return gx

    wd = w.cuda()
    dx = torch.full((B, 24, hin, win), float("nan"), device="cuda")
    want = torch.empty(B, 24, hin, win, dtype=torch.float64)
    keep = []
    for t in range(8):
        dzd = T.to_cb16(dz[t].cuda(), 128, 64).to(dt)
        keep.append(dzd)
        call(name, ptr(wd), ptr(dzd), I(128), I(64), I(hin), I(win), I(sf), ptr(dx), I(24), I(3 * t), I(0), I(B), stream())
        want[:, 3 * t:3 * t + 3] = ref(dz[t])
    dzd = T.to_cb16(dz[8].cuda(), 64, 0).to(dt)
    call(name, ptr(wd), ptr(dzd), I(64), I(0), I(hin), I(win), I(sf), ptr(dx), I(24), I(9), I(1), I(B), stream())
    torch.cuda.synchronize()
    got = dx.cpu().double()
    for t in range(8):
        exp = want[:, 3 * t:3 * t + 3] + (ref(dz[8]) if t == 3 else 0)
        e = relerr(got[:, 3 * t:3 * t + 3], exp)
        assert e < 1e-5, (t, e)
    # bit-reproducible: the same launch again gives the same bits
    dx2 = torch.empty(B, 3, hin, win, device="cuda")
    dx3 = torch.empty(B, 3, hin, win, device="cuda")
    for out in (dx2, dx3):
        call(name, ptr(wd), ptr(keep[0]), I(128), I(64), I(hin), I(win), I(sf), ptr(out), I(3), I(0), I(0), I(B), stream())
    assert torch.equal(dx2, dx3)


# ----------------------------------------------------------------------------------------------------- whole network
def oracle_input_grad(sd, LR, HR, sf, masks=None, emulate=None, front=None):
    """fp64 (or emulated) oracle: d mse / d LR with the ReLU pattern forced to `masks`; with `front` = (weight, bias) of a
    1x1 calibration conv in front of the network, the gradients of that conv's weight and bias instead."""
    dtype = torch.float32 if emulate else torch.float64
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = LR.to(dtype).requires_grad_(True)
    leaves = [x]
    inp = x
    if front is not None:
        fw, fb = (t.detach().cpu().to(dtype).requires_grad_(True) for t in front)
        leaves = [fw, fb]
        inp = F.conv2d(x, fw, fb)
    tap = O.ReluTap(masks=masks) if masks is not None else None
    out = O.tactilesr_forward(p, inp, scale_factor=sf, training=True, new_stats={}, tap=tap, emulate=emulate)
    return torch.autograd.grad(F.mse_loss(out, HR.to(dtype)), leaves)


def _model(T, cfg, sd, impl):
    m = T.TactileSR(**cfg)
    m.train_impl = impl
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    eng = m.train_engine()
    eng.keep_ctx = True
    return m, eng


def _data(cfg, B, seed):
    sf, Tn = cfg.get("scale_factor", 10), cfg.get("seqsCnt", 1)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), seed)
    g = torch.Generator().manual_seed(seed + 1)
    LR = torch.rand(B, 3 * Tn, 4, 4, generator=g) * 8
    HR = torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25
    return sd, LR, HR


CFGS = [(dict(), 3, 977), (dict(seqsCnt=2, patternFeatureExtraLayerCnt=1), 4, 978),
        (dict(seqsCnt=8, scale_factor=25, patternFeatureExtraLayerCnt=2), 2, 1977)]


@pytest.mark.parametrize("impl", ["fp16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("cfg,B,seed", CFGS)
def test_input_grad_vs_fp64_oracle_on_device_pattern(T, cfg, B, seed, impl):
    """LR.requires_grad_() -> MSE -> backward(): LR.grad against the fp64 oracle's on the device's ReLU pattern, max-norm
    1e-5 (2e-5 at sf 25, the parameter-gradient bars of the same steps).  Before this feature LR.grad stayed None."""
    sf = cfg.get("scale_factor", 10)
    sd, LR, HR = _data(cfg, B, seed)
    m, eng = _model(T, cfg, sd, impl)
    x = LR.cuda().requires_grad_(True)
    loss = F.mse_loss(m(x), HR.cuda())
    loss.backward()
    assert x.grad is not None and x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    (g64,) = oracle_input_grad(sd, LR, HR, sf, masks=masks)
    e = relerr(x.grad, g64)
    print(f"[input grad {impl} {cfg} B={B}] max-norm error {e:.2e} vs fp64 on the device's pattern")
    assert e < (2e-5 if sf == 25 else 1e-5), e
    assert all(p.grad is not None for p in m.parameters())


@pytest.mark.parametrize("impl", ["bf16", "bf16op"])
def test_input_grad_reduced_precision(T, impl):
    """bf16 / bf16op train arithmetic: LR.grad points the fp64 gradient's way (cosine > 0.98, the bar the parameter
    gradients of these modes meet); for bf16 the cosine against the bf16-emulating oracle is printed too."""
    cfg = dict(patternFeatureExtraLayerCnt=2)
    sd, LR, HR = _data(cfg, 4, 211)
    m, _ = _model(T, cfg, sd, impl)
    x = LR.cuda().requires_grad_(True)
    F.mse_loss(m(x), HR.cuda()).backward()
    (g64,) = oracle_input_grad(sd, LR, HR, 10)
    cos = cosine(x.grad, g64)
    msg = f"[input grad {impl}] cosine vs fp64 {cos:.5f}"
    if impl == "bf16":
        (ge,) = oracle_input_grad(sd, LR, HR, 10, emulate="bf16")
        msg += f", vs the bf16-emulating oracle {cosine(x.grad, ge):.5f}"
    print(msg)
    assert cos > 0.98, cos


def _step(T, cfg, sd, LR, HR, impl, requires_grad):
    m, _ = _model(T, cfg, sd, impl)
    m.train_engine().keep_ctx = False
    x = LR.cuda().requires_grad_(requires_grad)
    loss = F.mse_loss(m(x), HR.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}, \
        {k: v.clone() for k, v in m.state_dict().items() if "running" in k}, x.grad


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_input_grad_does_not_change_the_step(T, impl):
    """The same step with and without LR.requires_grad: bitwise-equal loss, parameter gradients and running statistics;
    without it LR.grad stays None; two runs with it give bitwise-equal LR.grad."""
    cfg = dict(seqsCnt=2, patternFeatureExtraLayerCnt=1)
    sd, LR, HR = _data(cfg, 5, 4242)
    l0, g0, s0, x0 = _step(T, cfg, sd, LR, HR, impl, False)
    l1, g1, s1, x1 = _step(T, cfg, sd, LR, HR, impl, True)
    l2, g2, s2, x2 = _step(T, cfg, sd, LR, HR, impl, True)
    assert x0 is None and x1 is not None
    assert torch.equal(l0, l1) and torch.equal(l1, l2)
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and torch.equal(g1[k], g2[k]), k
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert torch.equal(x1, x2)
    assert bool(torch.isfinite(x1).all()) and float(x1.abs().max()) > 0


def test_input_grad_routes_through_slices_dtypes_and_an_upstream_module(T):
    """autograd routes dx through the caller's graph: a slice of a wider leaf gets zeros in the other channels, an fp64
    leaf an fp64 grad, and a 1x1 calibration conv in front of the network the oracle's chained gradient."""
    cfg = dict()
    sd, LR, HR = _data(cfg, 3, 977)
    HRd = HR.cuda()
    # reference: plain fp32 leaf
    m, _ = _model(T, cfg, sd, "fp16x3")
    x = LR.cuda().requires_grad_(True)
    F.mse_loss(m(x), HRd).backward()
    ref = x.grad.clone()
    # a 6-channel leaf, the trainer's LR[:, :3]
    m, _ = _model(T, cfg, sd, "fp16x3")
    wide = torch.cat([LR, torch.rand(3, 3, 4, 4)], 1).cuda().requires_grad_(True)
    F.mse_loss(m(wide[:, :3]), HRd).backward()
    assert torch.equal(wide.grad[:, 3:], torch.zeros_like(wide.grad[:, 3:]))
    assert torch.equal(wide.grad[:, :3], ref)
    # an fp64 leaf
    m, _ = _model(T, cfg, sd, "fp16x3")
    x64 = LR.double().cuda().requires_grad_(True)
    F.mse_loss(m(x64), HRd).backward()
    assert x64.grad.dtype == torch.float64 and relerr(x64.grad, ref) < 1e-6
    # an upstream calibration layer on the device
    torch.manual_seed(5)
    cal = torch.nn.Conv2d(3, 3, 1).cuda()
    with torch.no_grad():
        cal.weight.copy_(torch.eye(3).view(3, 3, 1, 1) + 0.1 * torch.randn(3, 3, 1, 1))
        cal.bias.copy_(0.2 * torch.randn(3))
    m, eng = _model(T, cfg, sd, "fp16x3")
    F.mse_loss(m(cal(LR.cuda())), HRd).backward()
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    gw, gb = oracle_input_grad(sd, LR, HR, 10, masks=masks, front=(cal.weight, cal.bias))
    ew, eb = relerr(cal.weight.grad, gw), relerr(cal.bias.grad, gb)
    print(f"[input grad -> calibration conv] weight {ew:.2e}, bias {eb:.2e}")
    assert ew < 1e-5 and eb < 1e-5


def test_input_grad_B8192_tiling_invariance(T):
    """B = 8192 (fp16x3, sf 10) = 32 distinct (LR, HR) pairs tiled 256 times: the batch statistics equal the B = 32 run's,
    so LR.grad of copy k is the B = 32 run's LR.grad[k mod 32] x 32 / 8192 (MSE averages over the batch)."""
    torch.manual_seed(42)
    m = T.TactileSR().cuda()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(43)
    LR, HR = torch.rand(32, 3, 4, 4, generator=g) * 8, torch.rand(32, 1, 40, 40, generator=g) * 25

    def run(reps):
        m.load_state_dict(sd)
        m.train()
        x = LR.repeat(reps, 1, 1, 1).cuda().requires_grad_(True)
        F.mse_loss(m(x), HR.repeat(reps, 1, 1, 1).cuda()).backward()
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        return x.grad.detach()

    g32 = run(1).cpu()
    torch.cuda.empty_cache()
    g8k = run(256).view(256, 32, 3, 4, 4).cpu() * (8192 / 32)
    torch.cuda.empty_cache()
    e = float((g8k - g32.unsqueeze(0)).abs().max() / g32.abs().max())
    print(f"[input grad B=8192 tiled] max-norm deviation from the B=32 gradient {e:.2e}")
    assert e < 1e-5, e
