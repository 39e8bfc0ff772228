"""Per-kernel checks of the train step's glue kernels against fp64 torch references, through the C ABI with real buffers:
the stem and head weight gradients, the BatchNorm statistics / backward kernels, target preparation, MSE, PSNR / SSIM and
the layout converters.  The whole-network tests reach these kernels only at two image sizes and hold them to a
tensor-wide bar; here every output is checked on its own, at the shapes where the kernels switch their work split, LDS
footprint or tail handling.  bf16 variants get bf16-representable inputs, so the fp64 reference stays exact."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O

pytestmark = pytest.mark.gpu

SFS = [1, 2, 3, 5, 8, 16, 17, 28, 29, 31]


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd  # noqa: F401
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def bf(x):
    """Round to bf16 and back: an input the bf16 kernels store exactly."""
    return x.bfloat16().float()


def cb16(T, x, ctot, coff, b16):
    """NCHW (B, C, H, W) -> a CB16 buffer of ctot channels with x at coff (bf16 storage when b16)."""
    t = T.to_cb16(x.cuda(), ctot, coff)
    return t.bfloat16() if b16 else t


def from_cb16(T, t, B, C, H, W, ctot, coff):
    return T.from_cb16(t.float().contiguous(), B, C, H, W, ctot, coff)


def _status(name, *args):
    from tactilesr_amd import _lib
    return getattr(_lib.load(), name)(*args)


# ---------------------------------------------------------------------------------------------------- stem wgrad
@pytest.mark.parametrize("b16", [False, True])
@pytest.mark.parametrize("nsplit", [1, 2, 3, 8, 16, "B+1"])
@pytest.mark.parametrize("sf", SFS)
def test_stem_wgrad_vs_fp64_autograd(T, sf, nsplit, b16):
    """dW of conv3x3(interpolate(x, x sf)) from the frame at lr_coff = 3t of a 24-channel taxel tensor and the 64 dz channels
    at dz_coff of a CB16 tensor; the nsplit slab entries summed within 1e-5 of fp64.  Odd B: every band / split rule,
    divisible or not (sf 29 .. 31 at nsplit 1 / 3 / B+1 was refused before the bands stopped depending on nsplit)."""
    from tactilesr_amd._lib import ptr, stream, c_int as I
    B, hin = 3, 4
    H = W = hin * sf
    ns = B + 1 if nsplit == "B+1" else nsplit
    t = (sf + ns) % 8
    dz_ctot, dz_coff = (128, 64) if ns % 2 else (64, 0)
    g = torch.Generator().manual_seed(100 * sf + ns + int(b16))
    lr = torch.rand(B, 24, hin, hin, generator=g) * 8
    dz = torch.randn(B, 64, H, W, generator=g)
    if b16:
        dz = bf(dz)
    x = lr[:, 3 * t:3 * t + 3].double()
    w = torch.zeros(64, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    z = F.conv2d(F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False), w, padding=1)
    (ref,) = torch.autograd.grad(z, w, dz.double())
    dzd = cb16(T, dz, dz_ctot, dz_coff, b16)
    lrd = lr.cuda()
    slab = torch.full((ns, 64 * 27), float("nan"), device="cuda")
    st = _status("tsr_stem_wgrad_b16" if b16 else "tsr_stem_wgrad", ptr(lrd), I(24), I(3 * t), I(hin), I(hin), I(sf),
                 ptr(dzd), I(dz_ctot), I(dz_coff), ptr(slab), I(ns), I(B), stream())
    assert st == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(slab).all())           # every one of the nsplit entries written
    got = slab.double().sum(0).view(64, 3, 3, 3)
    e = relerr(got, ref)
    assert e < 1e-5, e


def test_stem_wgrad_refuses_an_image_beyond_lds_before_any_launch(T):
    """A row of 3 x (W + 2) floats per band row that cannot fit 160 KB even in 1-row bands: status 1, slab untouched."""
    from tactilesr_amd._lib import ptr, stream, c_int as I
    lr = torch.zeros(1, 3, 1, 4400, device="cuda")
    dz = torch.zeros(64, device="cuda")                 # never read
    slab = torch.full((1, 64 * 27), 7.0, device="cuda")
    assert _status("tsr_stem_wgrad", ptr(lr), I(3), I(0), I(1), I(4400), I(1), ptr(dz), I(64), I(0), ptr(slab), I(1), I(1),
                   stream()) == 1
    torch.cuda.synchronize()
    assert bool((slab == 7.0).all())


# ------------------------------------------------------------------------------------------------------ head bwd
HEAD_HW = [(4, 4), (8, 8), (9, 17), (40, 40), (64, 64), (68, 68), (124, 124)]


@pytest.mark.parametrize("b16", [False, True])
@pytest.mark.parametrize("nsplit", [1, 3, 5])
@pytest.mark.parametrize("cin", [64, 128, 256])
@pytest.mark.parametrize("H,W", HEAD_HW)
def test_head_bwd_vs_fp64_autograd(T, H, W, cin, nsplit, b16):
    """out = relu(conv3x3(h0, w)), h0 post-ReLU (CB16, h_ctot > cin): dz_h0 = conv^T(dout [out > 0]) [h0 > 0] elementwise vs
    fp64, the channels past cin of dz_h0 untouched, the nsplit (1, 3, > B) weight partials summed within 1e-5, and
    dz_amax == max|dz_h0| exactly (fp32 form)."""
    from tactilesr_amd._lib import ptr, stream, c_int as I
    B = 3
    h_ctot, dz_ctot = cin + 64, cin + 32
    g = torch.Generator().manual_seed(H * 1000 + W + cin + nsplit + int(b16))
    h0 = F.relu(torch.randn(B, cin, H, W, generator=g))
    if b16:
        h0 = bf(h0)
    w = torch.randn(1, cin, 3, 3, generator=g) * 0.1
    out = F.relu(torch.randn(B, 1, H, W, generator=g))
    dout = torch.randn(B, 1, H, W, generator=g)
    dp = (dout * (out > 0)).double()
    hh = h0.double().requires_grad_(True)
    ww = w.double().requires_grad_(True)
    gh, gw = torch.autograd.grad(F.conv2d(hh, ww, padding=1), [hh, ww], dp)
    ref_dz = gh * (h0 > 0)
    h0d = cb16(T, h0, h_ctot, 0, b16)
    dzd = torch.full((B * dz_ctot * H * W,), 3.0, device="cuda")
    dzd = dzd.bfloat16() if b16 else dzd
    wslab = torch.full((nsplit, cin * 9), float("nan"), device="cuda")
    amax = torch.zeros(1, device="cuda")
    wd, doutd, outd = w.cuda(), dout.cuda(), out.cuda()
    if b16:
        st = _status("tsr_head_bwd_b16", ptr(doutd), ptr(outd), ptr(h0d), I(h_ctot), I(cin), ptr(wd), ptr(dzd), I(dz_ctot),
                     ptr(wslab), I(nsplit), I(B), I(H), I(W), stream())
    else:
        st = _status("tsr_head_bwd", ptr(doutd), ptr(outd), ptr(h0d), I(h_ctot), I(cin), ptr(wd), ptr(dzd), I(dz_ctot),
                     ptr(wslab), I(nsplit), I(B), I(H), I(W), ptr(amax), stream())
    assert st == 0
    torch.cuda.synchronize()
    got = from_cb16(T, dzd, B, cin, H, W, dz_ctot, 0).cpu().double()
    rest = from_cb16(T, dzd, B, dz_ctot - cin, H, W, dz_ctot, cin)
    assert bool((rest == 3.0).all())
    mx = float(ref_dz.abs().max())
    if b16:     # one bf16 rounding of the fp32 result
        bad = (got - ref_dz).abs() > ref_dz.abs() * 2.0 ** -8 + 1e-6 * mx
    else:
        bad = (got - ref_dz).abs() > 1e-5 * mx
    assert not bool(bad.any()), (int(bad.sum()), float((got - ref_dz).abs().max()) / mx)
    e = relerr(wslab.double().sum(0).view(1, cin, 3, 3), gw)
    assert e < 1e-5, e
    if not b16:
        assert float(amax) == float(got.abs().max())


@pytest.mark.parametrize("b16", [False, True])
def test_head_bwd_refuses_oversize_before_any_launch(T, b16):
    """128 x 128 (sf 32): the padded image is over the 64 KB LDS bound of the weight-gradient kernel.  Status 1, and a
    sentinel-filled dz_h0 / wslab / dz_amax stay untouched (no launch of the data-gradient kernel either)."""
    from tactilesr_amd._lib import ptr, stream, c_int as I
    B, H, W, cin = 1, 128, 128, 128
    h0 = torch.ones(B * cin * H * W, device="cuda")
    dz = torch.full((B * cin * H * W,), 5.0, device="cuda")
    if b16:
        h0, dz = h0.bfloat16(), dz.bfloat16()
    w = torch.ones(cin * 9, device="cuda")
    dout = torch.ones(B * H * W, device="cuda")
    wslab = torch.full((cin * 9,), 5.0, device="cuda")
    amax = torch.full((1,), 5.0, device="cuda")
    if b16:
        st = _status("tsr_head_bwd_b16", ptr(dout), ptr(dout), ptr(h0), I(cin), I(cin), ptr(w), ptr(dz), I(cin),
                     ptr(wslab), I(1), I(B), I(H), I(W), stream())
    else:
        st = _status("tsr_head_bwd", ptr(dout), ptr(dout), ptr(h0), I(cin), I(cin), ptr(w), ptr(dz), I(cin), ptr(wslab),
                     I(1), I(B), I(H), I(W), ptr(amax), stream())
    assert st == 1
    torch.cuda.synchronize()
    assert bool((dz.float() == 5.0).all()) and bool((wslab == 5.0).all()) and float(amax) == 5.0


# ------------------------------------------------------------------------------------------------- BN statistics
@pytest.mark.parametrize("momentum", [0.1, 0.3])
@pytest.mark.parametrize("cond", [1.0, 1e2, 1e3])
@pytest.mark.parametrize("b16", [False, True])
@pytest.mark.parametrize("HW", [16, 63, 64, 65, 1600, 15376])
def test_cb16_stats_and_bn_stats_finalize_vs_fp64(T, HW, b16, cond, momentum):
    """Welford slabs of a 64-channel CB16 slice (z_coff 64 of 192) -> BatchNorm scale / shift / xhat_a / xhat_b and the
    running-statistics update (conv bias on the mean, unbiased N/(N-1) variance) against fp64 formulas, per channel
    within 1e-5.  `cond` = |mean| / std of every channel (mean of either sign, std spread over 1e-2 .. 1e2).

    At cond 1e3 the bar is 5e-5 (measured worst 3.0e-5: scale at HW = 16).  Cause: the slab holds each entry's mean in
    fp32, a few ulp of |mean| off the entry's exact mean after the fp32 sum and merges (d_e ~ 1e-4 std at cond 1e3); the
    batch variance formed from (mean_e, M2_e) then carries 2 (mean_e - mean) d_e / E, ~3e-5 of the variance with E = 3
    entries and shrinking as 1/sqrt(E) (1.6e-6 at HW = 1600).  A double merge of corrected two-pass partials removes it
    but moves the rounding of every stem BatchNorm in the train step; the conv epilogues' slabs share the format."""
    from tactilesr_amd._lib import ptr, stream, call, c_int as I, c_float as Fl
    from tactilesr_amd import _lib
    B, C = 3, 64
    g = torch.Generator().manual_seed(HW + int(1e3 * momentum) + int(cond) + int(b16))
    std = 10.0 ** (torch.rand(C, generator=g) * 4 - 2)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    z = (torch.randn(B, C, HW, generator=g) * std.view(1, C, 1) + (sign * cond * std).view(1, C, 1))
    if b16:
        z = bf(z)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    bias = torch.randn(C, generator=g) * std
    rm0, rv0 = torch.randn(C, generator=g) * std, torch.rand(C, generator=g) * std * std + 0.1
    eps = 1e-5
    zd = cb16(T, z.view(B, C, HW, 1), 192, 64, b16)
    entries = _lib.load().tsr_cb16_stats_entries(B, HW)
    slab = torch.empty(entries * C * 2, device="cuda")
    cnt = torch.empty(entries, device="cuda")
    call("tsr_cb16_stats_b16" if b16 else "tsr_cb16_stats", ptr(zd), I(192), I(64), I(B), I(HW), ptr(slab), ptr(cnt),
         stream())
    rm, rv = rm0.cuda(), rv0.cuda()
    outs = [torch.empty(C, device="cuda") for _ in range(4)]
    work = torch.empty(512 * C * 3, dtype=torch.float64, device="cuda")
    vec = [v.cuda() for v in (bias, gamma, beta)]        # (held: a temporary's memory could back the next one)
    call("tsr_bn_stats_finalize", ptr(slab), ptr(cnt), I(entries), I(C), *[ptr(v) for v in vec], ptr(rm), ptr(rv), Fl(momentum), Fl(eps), *[ptr(o) for o in outs], ptr(work), stream())
    torch.cuda.synchronize()
    zz = z.double()
    N = B * HW
    mean = zz.mean(dim=(0, 2))
    var = zz.var(dim=(0, 2), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    sc = gamma.double() * invstd
    ref = {"scale": (sc, sc.abs()),
           "shift": (beta.double() - mean * sc, beta.double().abs() + (mean * sc).abs()),
           "xhat_a": (invstd, invstd),
           "xhat_b": (-mean * invstd, (mean * invstd).abs()),
           "running_mean": ((1 - momentum) * rm0.double() + momentum * (mean + bias.double()),
                            (1 - momentum) * rm0.double().abs() + momentum * (mean.abs() + bias.double().abs())),
           "running_var": ((1 - momentum) * rv0.double() + momentum * var * N / (N - 1), None)}
    got = dict(zip(["scale", "shift", "xhat_a", "xhat_b"], outs), running_mean=rm, running_var=rv)
    tol = 5e-5 if cond >= 1e3 else 1e-5
    for k, (r, mag) in ref.items():
        mag = r.abs() if mag is None else mag
        e = float(((got[k].cpu().double() - r).abs() / mag).max())
        assert e < tol, (k, e)


# --------------------------------------------------------------------------------------------------- BN backward
@pytest.mark.parametrize("b16", [False, True])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("entries", [1, 2, 3, 511, 512, 1023, 1025, 4097])
def test_bn_bwd_finalize_and_apply_vs_fp64_batchnorm_backward(T, entries, C, b16):
    """epi_mode-2 slabs (per entry and channel: sum g, sum g*xhat over that entry's share of the B*HW elements) with
    `entries` around the tails of the two-chain reduction loop -> dgamma, dbeta and the applied dz = c1 g + c2 z + c3
    (in place on a CB16 slice) against torch's fp64 BatchNorm backward; out_amax == max|dz| exactly (fp32 form)."""
    from tactilesr_amd._lib import ptr, stream, call, c_int as I, c_double as D
    B = 2
    HW = max(64, (entries + B - 1) // B + 7)
    N = B * HW
    g0 = torch.Generator().manual_seed(entries * 7 + C + int(b16))
    z = torch.randn(B, C, HW, generator=g0) * 2 + 0.5
    gy = torch.randn(B, C, HW, generator=g0)
    if b16:
        z, gy = bf(z), bf(gy)
    gamma, beta, eps = torch.rand(C, generator=g0) + 0.5, torch.randn(C, generator=g0), 1e-5
    zz = z.double()
    mean, var = zz.mean(dim=(0, 2)), zz.var(dim=(0, 2), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale, xa, xb = (gamma.double() * invstd).float(), invstd.float(), (-mean * invstd).float()
    xhat = zz * xa.double().view(1, C, 1) + xb.double().view(1, C, 1)
    # slabs: the N elements of a channel in `entries` contiguous shares
    flat_g = gy.double().permute(1, 0, 2).reshape(C, N)
    flat_gx = (gy.double() * xhat).permute(1, 0, 2).reshape(C, N)
    slab = torch.stack([torch.stack([a.sum(1), b.sum(1)], 1)
                        for a, b in zip(flat_g.tensor_split(entries, 1), flat_gx.tensor_split(entries, 1))]).float()
    dgamma, dbeta, c1, c2, c3 = (torch.empty(C, device="cuda") for _ in range(5))
    work = torch.empty(512 * C * 3, dtype=torch.float64, device="cuda")
    dev = [v.cuda().contiguous() for v in (slab, scale, xa, xb)]
    call("tsr_bn_bwd_finalize", ptr(dev[0]), I(entries), I(C), D(float(N)), *[ptr(v) for v in dev[1:]], ptr(dgamma), ptr(dbeta), ptr(c1), ptr(c2), ptr(c3), ptr(work), stream())
    ctot, coff = C + 32, 16
    gd = cb16(T, gy.view(B, C, HW, 1), ctot, coff, b16)
    zd = cb16(T, z.view(B, C, HW, 1), C + 64, 64, b16)
    amax = torch.zeros(1, device="cuda")
    if b16:
        call("tsr_bn_bwd_apply_b16", ptr(gd), I(ctot), I(coff), ptr(zd), I(C + 64), I(64), ptr(c1), ptr(c2), ptr(c3), I(C),
             I(B), I(HW), stream())
    else:
        call("tsr_bn_bwd_apply", ptr(gd), I(ctot), I(coff), ptr(zd), I(C + 64), I(64), ptr(c1), ptr(c2), ptr(c3), I(C),
             I(B), I(HW), ptr(amax), stream())
    torch.cuda.synchronize()
    # fp64 reference: torch's BatchNorm backward in training mode
    x = zz.view(B, C, HW, 1).clone().requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.batch_norm(x, None, None, gm, bt, training=True, eps=eps)
    rdx, rdg, rdb = torch.autograd.grad(y, [x, gm, bt], gy.double().view(B, C, HW, 1))
    # per channel: the exact sum of the fp32 partials handed in within 1e-6, and torch's within 1e-5 of the channel's
    # sum of magnitudes (the partials' own fp32 rounding is what separates the two)
    mag = {"dgamma": flat_gx.abs().sum(1), "dbeta": flat_g.abs().sum(1)}
    for j, (k, got, ref) in enumerate((("dgamma", dgamma, rdg), ("dbeta", dbeta, rdb))):
        got = got.cpu().double()
        exact = slab.double()[:, :, 1 - j].sum(0)
        e1 = float(((got - exact).abs() / exact.abs().clamp_min(1e-3 * float(exact.abs().max()))).max())
        e2 = float(((got - ref).abs() / mag[k]).max())
        assert e1 < 1e-6 and e2 < 1e-5, (k, e1, e2)
    dz = from_cb16(T, gd, B, C, HW, 1, ctot, coff).cpu().double().view(B, C, HW)
    ref = rdx.view(B, C, HW)
    mxc = ref.abs().amax(dim=(0, 2)).view(1, C, 1)             # per channel
    if b16:
        bad = (dz - ref).abs() > ref.abs() * 2.0 ** -8 + 1e-5 * mxc
    else:
        bad = (dz - ref).abs() > 1e-5 * mxc
    assert not bool(bad.any()), (int(bad.sum()), float(((dz - ref).abs() / mxc).max()))
    if not b16:
        assert float(amax) == float(dz.abs().max())


# ----------------------------------------------------------------------------------------- target, loss, metrics
@pytest.mark.parametrize("hw,out_hw", [((100, 100), (4 * sf, 4 * sf)) for sf in SFS] + [((100, 60), (68, 36))])
def test_target_prep_vs_fp64_interpolate(T, hw, out_hw):
    """HR / HR_scale_num + bilinear (align_corners=False) resize, up or down, square or not, against torch's resize."""
    from tactilesr_amd._lib import ptr, stream, call, c_int as I, c_float as Fl
    B = 3
    hr = torch.rand(B, 1, *hw, generator=torch.Generator().manual_seed(out_hw[0] + hw[1])) * 250
    out = torch.empty(B, 1, *out_hw, device="cuda")
    hrd = hr.cuda()
    call("tsr_target_prep", ptr(hrd), ptr(out), Fl(1.0 / 10.0), I(B), I(hw[0]), I(hw[1]), I(out_hw[0]), I(out_hw[1]),
         stream())
    # the reference's own fp32 resize within 1e-6; fp64 within 1e-5: both form the source coordinate scale * (dst + 0.5)
    # - 0.5 in fp32 (scale = hin / H rounded), up to 6e-6 of a pixel at 100 rows, which moves a random image by that much
    ref32 = F.interpolate(hr / 10.0, size=out_hw, mode="bilinear", align_corners=False)
    ref64 = F.interpolate(hr.double() / 10.0, size=out_hw, mode="bilinear", align_corners=False)
    e32, e64 = relerr(out, ref32), relerr(out, ref64)
    assert e32 < 1e-6 and e64 < 1e-5, (e32, e64)


@pytest.mark.parametrize("with_dy", [True, False])
@pytest.mark.parametrize("n", [1, 255, 257, 16 * 17 * 17 * 3, 16 * 31 * 31 * 5])
def test_mse_fwd_bwd_vs_fp64(T, n, with_dy):
    """loss = mean (y - t)^2 and dy = grad_scale * 2 (y - t) / n (grad_scale 0.37), dy = NULL allowed."""
    from tactilesr_amd._lib import ptr, stream, call, c_float as Fl, c_longlong as L
    g = torch.Generator().manual_seed(n)
    y, t = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g) * 3
    dy = torch.full((n,), float("nan"), device="cuda") if with_dy else None
    loss = torch.empty(1, device="cuda")
    work = torch.empty(256, dtype=torch.float64, device="cuda")
    yd, td = y.cuda(), t.cuda()
    call("tsr_mse_fwd_bwd", ptr(yd), ptr(td), ptr(dy), ptr(loss), L(n), Fl(0.37), ptr(work), stream())
    d = y.double() - t.double()
    assert abs(float(loss) - float((d * d).mean())) <= 1e-6 * float((d * d).mean())
    if with_dy:
        e = relerr(dy, 0.37 * 2 * d / n)
        assert e < 1e-6, e


@pytest.mark.parametrize("sf", [3, 17, 31])
def test_psnr_ssim_vs_fp64(T, sf):
    """Per-sample PSNR (psnr_div = 4sf, the reference's (1, H, W) quirk) and single-window SSIM for n = 16 sf^2 (not a
    multiple of 256), odd B, against the oracle's formulas in fp64."""
    from tactilesr_amd._lib import ptr, stream, call, c_int as I, c_double as D
    B, H = 5, 4 * sf
    n = H * H
    g = torch.Generator().manual_seed(sf)
    a = torch.rand(B, 1, H, H, generator=g) * 25
    b = (a + torch.randn(B, 1, H, H, generator=g)).clamp_min(0)
    ps, ss = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ad, bd = a.cuda(), b.cuda()
    call("tsr_psnr_ssim", ptr(ad), ptr(bd), I(B), I(n), D(float(H)), D(250.0), D(C1), D(C2), ptr(ps), ptr(ss),
         stream())
    for i in range(B):
        rp = float(O.calculation_psnr(a[i].double(), b[i].double(), 250.0))
        rs = float(O.calculation_ssim(a[i].double(), b[i].double(), C1, C2))
        assert abs(float(ps[i]) - rp) <= 1e-5 * abs(rp) and abs(float(ss[i]) - rs) <= 1e-5 * abs(rs), (i, rp, rs)


# ------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("B,C,HW,ctot,coff", [(3, 64, 16, 64, 0), (2, 48, 1600, 128, 80), (1, 16, 15376, 192, 176),
                                              (5, 3, 63, 16, 0), (2, 24, 65, 64, 32)])
def test_nchw_cb16_round_trip_is_bit_exact(T, B, C, HW, ctot, coff):
    """NCHW -> a channel slice of CB16 -> NCHW returns the same bits, the layout is [B][ctot/16][HW][16], and the channels
    outside the slice keep their contents."""
    from tactilesr_amd._lib import ptr, stream, call, c_int as I
    x = torch.randn(B, C, HW, generator=torch.Generator().manual_seed(HW + C)).cuda()
    buf = torch.full((B * ctot * HW,), -1.5, device="cuda")
    call("tsr_nchw_to_cb16", ptr(x), ptr(buf), I(B), I(C), I(HW), I(ctot), I(coff), stream())
    back = torch.empty(B, C, HW, device="cuda")
    call("tsr_cb16_to_nchw", ptr(buf), ptr(back), I(B), I(C), I(HW), I(ctot), I(coff), stream())
    assert torch.equal(back, x)
    v = buf.view(B, ctot // 16, HW, 16).permute(0, 1, 3, 2).reshape(B, ctot, HW)
    assert torch.equal(v[:, coff:coff + C], x)
    keep = torch.ones(ctot, dtype=torch.bool)
    keep[coff:coff + C] = False
    assert bool((v[:, keep] == -1.5).all())
