"""GPU parity of the training path: wgrad / dgrad kernels against torch autograd on CPU, and the
whole train-mode forward + backward (+ Adam) against the reference's own run (tests/golden/train.npz)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O
import _gradcheck as GC

pytestmark = pytest.mark.gpu


def _debug_engine(m):
    """Create the module's train engine with `keep_ctx` armed (forward then keeps its context alive so the test can
    read the activation pattern back)."""
    eng = m.train_engine()
    eng.keep_ctx = True
    return eng


def relerr(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


@pytest.mark.parametrize("impl", ["f32", "bf16x6", "fp16x3"])
@pytest.mark.parametrize("ks,cin,cout,B,H,W,affine", [
    (3, 64, 64, 3, 40, 40, False), (5, 64, 64, 2, 40, 40, True), (3, 128, 128, 2, 40, 40, True),
    (5, 128, 128, 2, 16, 24, False), (1, 256, 64, 3, 40, 40, True), (3, 128, 64, 5, 13, 21, True),
])
def test_conv2d_wgrad(T, ks, cin, cout, B, H, W, affine, impl):
    from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_float as Fl, c_longlong as L
    g = torch.Generator().manual_seed(ks + cin + cout + B)
    araw = torch.randn(B, cin, H, W, generator=g)
    dz = torch.randn(B, cout, H, W, generator=g)
    if impl == "fp16x3":        # gradient-like dynamic range: tiny values with a few large outliers
        dz = dz * 1e-4
        dz[0, 0, 0, 0] = 0.37
        araw[0, 1, 2, 3] = 41.0
    sc = torch.rand(cin, generator=g) + 0.5
    sh = torch.randn(cin, generator=g) * 0.3
    a = F.relu(araw * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if affine else araw
    w = torch.zeros(cout, cin, ks, ks, requires_grad=True)
    y = F.conv2d(a, w, padding=ks // 2)
    (gw,) = torch.autograd.grad(y, w, dz)
    gb = dz.sum(dim=(0, 2, 3))
    ad, dzd = T.to_cb16(araw.cuda(), cin + 16, 16), T.to_cb16(dz.cuda(), cout + 32, 16)
    scd, shd = (sc.cuda(), sh.cuda()) if affine else (None, None)
    ns = min(B, 3)
    n = cout * cin * ks * ks
    slab = torch.empty(ns * n, device="cuda")
    bslab = torch.empty(ns * cout, device="cuda")
    if impl == "f32":
        call("tsr_conv2d_wgrad", ptr(ad), I(cin + 16), I(16), I(cin), ptr(scd), ptr(shd), ptr(dzd), I(cout + 32), I(16),
             I(cout), I(ks), ptr(slab), ptr(bslab), I(ns), I(B), I(H), I(W), stream())
    else:
        am = torch.stack([araw.abs().max(), dz.abs().max()]).cuda()      # producers publish these in the engine
        call("tsr_conv2d_wgrad_bf16s", ptr(ad), I(cin + 16), I(16), I(cin), ptr(scd), ptr(shd), ptr(dzd), I(cout + 32),
             I(16), I(cout), I(ks), I(3 if impl == "bf16x6" else -2), ptr(am[0:1]), ptr(am[1:2]), ptr(slab),
             ptr(bslab), I(ns), I(B), I(H), I(W), stream())
    out = torch.empty(cout, cin, ks, ks, device="cuda")
    outb = torch.empty(cout, device="cuda")
    call("tsr_reduce_splits", ptr(slab), ptr(out), L(n), I(ns), Fl(1.0), stream())
    call("tsr_reduce_splits", ptr(bslab), ptr(outb), L(cout), I(ns), Fl(1.0), stream())
    assert relerr(out, gw) < 1e-5
    assert relerr(outb, gb) < 1e-5


@pytest.mark.parametrize("ks,cin,cout,B,H,W,affine,ns", [
    (3, 64, 64, 3, 40, 40, False, 3), (5, 64, 64, 2, 40, 40, False, 2), (3, 128, 128, 2, 40, 40, False, 7),
    (5, 128, 128, 2, 16, 24, False, 5), (3, 128, 64, 5, 13, 21, False, 4), (5, 128, 128, 3, 13, 21, False, 1),
    (5, 64, 128, 1, 5, 3, False, 2), (3, 256, 128, 2, 40, 40, False, 11), (5, 128, 128, 2, 40, 40, True, 3),
    (3, 128, 128, 2, 13, 21, True, 2), (1, 256, 64, 3, 40, 40, True, 3), (1, 256, 64, 2, 13, 21, False, 2),
])
def test_conv2d_wgrad_bf16_storage(T, ks, cin, cout, B, H, W, affine, ns):
    """Training with bf16 activation storage: the weight / bias gradient from bf16 CB16 tensors (tsr_conv2d_wgrad_bf16s,
    planes = -1).  Launches without a fused input transform run csrc/wgrad_b16k.hip (LDS-DMA staging), the others
    wgrad_mfma_tr16.hip.  Yardstick: torch autograd in fp64 on the bf16-ROUNDED operands (with `affine`, the input is
    bf16(relu(z * scale + shift)) of the stored bf16 z, fp32 arithmetic, as the kernel forms it): products of bf16 values
    are exact in fp32, so what is left is fp32 summation order -- 1e-5 of the gradient's scale.  Ragged images (13 x 21,
    5 x 3), channel offsets into wider tensors and split counts that do not divide the items are part of the cases."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_float as Fl, c_longlong as L
    g = torch.Generator().manual_seed(ks * 3 + cin + cout + B + H)
    q = lambda t: t.bfloat16().float()
    araw = q(torch.randn(B, cin, H, W, generator=g))
    dz = q(torch.randn(B, cout, H, W, generator=g))
    sc = torch.rand(cin, generator=g) + 0.5
    sh = torch.randn(cin, generator=g) * 0.3
    a = q(F.relu(torch.addcmul(sh.view(1, -1, 1, 1), araw, sc.view(1, -1, 1, 1)))) if affine else araw
    w = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a.double(), w, padding=ks // 2)
    (gw,) = torch.autograd.grad(y, w, dz.double())
    gb = dz.double().sum(dim=(0, 2, 3))
    ad = T.to_cb16(araw.cuda(), cin + 16, 16).to(torch.bfloat16)
    dzd = T.to_cb16(dz.cuda(), cout + 32, 16).to(torch.bfloat16)
    scd, shd = (sc.cuda(), sh.cuda()) if affine else (None, None)
    n = cout * cin * ks * ks
    slab = torch.full((ns * n,), float("nan"), device="cuda")
    bslab = torch.full((ns * cout,), float("nan"), device="cuda")
    call("tsr_conv2d_wgrad_bf16s", ptr(ad), I(cin + 16), I(16), I(cin), ptr(scd), ptr(shd), ptr(dzd), I(cout + 32),
         I(16), I(cout), I(ks), I(-1), None, None, ptr(slab), ptr(bslab), I(ns), I(B), I(H), I(W), stream())
    out = torch.empty(cout, cin, ks, ks, device="cuda")
    outb = torch.empty(cout, device="cuda")
    call("tsr_reduce_splits", ptr(slab), ptr(out), L(n), I(ns), Fl(1.0), stream())
    call("tsr_reduce_splits", ptr(bslab), ptr(outb), L(cout), I(ns), Fl(1.0), stream())
    e, eb = relerr(out, gw), relerr(outb, gb)
    print(f"[bf16 wgrad] k{ks} {cin}->{cout} B={B} {H}x{W} affine={affine} ns={ns}: dW {e:.1e}, db {eb:.1e}")
    assert e < 1e-5 and eb < 1e-5
    if affine and T._lib.load().tsr_conv2d_wgrad_b16k(cout, cin, ks):
        # what the train engine does with a virtual input: materialise it once (tsr_bn_relu_b16 -- bit-identical to
        # bf16(relu(fma(z, scale, shift)))), then the launch without a transform (csrc/wgrad_b16k.hip)
        mat = torch.full((B * cin * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
        call("tsr_bn_relu_b16", ptr(ad), I(cin + 16), I(16), I(cin), ptr(scd), ptr(shd), ptr(mat), I(B), I(H * W), stream())
        assert torch.equal(T.from_cb16(mat, B, cin, H, W).float().cpu(), a)
        slab.fill_(float("nan")); bslab.fill_(float("nan"))
        call("tsr_conv2d_wgrad_bf16s", ptr(mat), I(cin), I(0), I(cin), None, None, ptr(dzd), I(cout + 32),
             I(16), I(cout), I(ks), I(-1), None, None, ptr(slab), ptr(bslab), I(ns), I(B), I(H), I(W), stream())
        call("tsr_reduce_splits", ptr(slab), ptr(out), L(n), I(ns), Fl(1.0), stream())
        call("tsr_reduce_splits", ptr(bslab), ptr(outb), L(cout), I(ns), Fl(1.0), stream())
        assert relerr(out, gw) < 1e-5 and relerr(outb, gb) < 1e-5


@pytest.mark.parametrize("ks,cin,cout,B,H,W,NP", [(3, 64, 64, 3, 40, 40, 64), (5, 128, 128, 2, 16, 24, 64),
                                                  (1, 256, 64, 2, 40, 40, 64), (3, 448, 64, 1, 40, 40, 64),
                                                  (1, 256, 64, 1, 40, 40, 128), (1, 256, 64, 3, 40, 40, 128),
                                                  (5, 128, 128, 5, 16, 24, 128), (3, 128, 128, 1, 40, 40, 128)])
def test_conv2d_dgrad_with_mask_and_bn_sums(T, ks, cin, cout, B, H, W, NP):
    """dgrad = conv with flipped/transposed weights; epilogue: + residual, ReLU mask by relu(bn(z)),
    BatchNorm-backward sums; then the elementwise BN backward -> compare with autograd."""
    from tactilesr_amd.model._train import conv_ex, Act, _pack_dgrad
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_double as D
    g = torch.Generator().manual_seed(ks + cin)
    z = torch.randn(B, cin, H, W, generator=g)
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
    dy = torch.randn(B, cout, H, W, generator=g)
    extra = torch.randn(B, cin, H, W, generator=g) * 0.1
    zr = z.clone().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = F.relu(F.batch_norm(zr, None, None, gm, bt, True, 0.1, 1e-5))
    y = F.conv2d(a, w, padding=ks // 2)
    loss = (y * dy).sum() + (a * extra).sum()
    gz, ggm, gbt = torch.autograd.grad(loss, (zr, gm, bt))
    mean = z.mean(dim=(0, 2, 3))
    var = z.var(dim=(0, 2, 3), unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    vec = torch.stack([gamma * invstd, beta - mean * gamma * invstd, invstd, -mean * invstd]).cuda()
    zd, dyd, exd = T.to_cb16(z.cuda()), T.to_cb16(dy.cuda()), T.to_cb16(extra.cuda())
    gbuf = torch.empty(B * cin * H * W, device="cuda")
    lib = load()
    entries = lib.tsr_conv2d_slab_entries_ex(B, H, W, NP, ks, 0)        # fp32-MFMA dgrad here (nsplit = 0)
    work = torch.empty(512 * 128 * 3, dtype=torch.float64, device="cuda")
    wd = w.cuda().contiguous()
    dgam, dbet = [], []
    for o in range(0, cin, NP):
        slab = torch.empty(entries * NP * 2, device="cuda")
        wp = _pack_dgrad(wd, cout, cin, ks, o, NP)
        mk = Act(zd, cin, o, NP, vec[0, o:o + NP], vec[1, o:o + NP], vec[2, o:o + NP], vec[3, o:o + NP])
        conv_ex(B=B, H=H, W=W, src=Act(dyd, cout, 0, cout), w=wp, cout=NP, ks=ks, out=gbuf, out_ctot=cin, out_coff=o,
                res=Act(exd, cin, o, NP), epi_mode=2, mask=mk, bn=True, slab=slab)
        out = torch.empty(5, NP, device="cuda")
        call("tsr_bn_bwd_finalize", ptr(slab), I(entries), I(NP), D(float(B * H * W)), ptr(vec[0, o:o + NP]),
             ptr(vec[2, o:o + NP]), ptr(vec[3, o:o + NP]), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
             ptr(out[4]), ptr(work), stream())
        am = torch.zeros(1, device="cuda")
        call("tsr_bn_bwd_apply", ptr(gbuf), I(cin), I(o), ptr(zd), I(cin), I(o), ptr(out[2]), ptr(out[3]), ptr(out[4]),
             I(NP), I(B), I(H * W), ptr(am), stream())
        assert am.item() == T.from_cb16(gbuf, B, cin, H, W)[:, o:o + NP].abs().max().item()
        dgam.append(out[0].clone())
        dbet.append(out[1].clone())
    assert relerr(T.from_cb16(gbuf, B, cin, H, W), gz) < 1e-5
    assert relerr(torch.cat(dgam), ggm) < 1e-5
    assert relerr(torch.cat(dbet), gbt) < 1e-5


@pytest.mark.parametrize("ks,cin,cout,B,H,W,res", [(5, 128, 128, 5, 16, 24, True), (3, 128, 128, 1, 40, 40, True),
                                                    (3, 256, 64, 3, 13, 21, False), (5, 128, 96, 2, 40, 40, True),
                                                    (1, 256, 64, 3, 13, 21, False), (1, 256, 64, 2, 40, 40, False),
                                                    (1, 128, 64, 70, 12, 12, False), (3, 64, 64, 5, 13, 21, True),
                                                    (5, 128, 64, 2, 40, 40, True), (3, 192, 96, 3, 16, 24, False)])
def test_conv2d_dgrad_bf16_storage_b16k(T, ks, cin, cout, B, H, W, res):
    """Training with bf16 activation storage: the dgrad launches of the 128-input-channel 3x3 / 5x5 layers run
    csrc/conv_b16k.hip (tsr_conv2d_ex, nsplit = -3, epi_mode = 2; weights from tsr_pack_conv_weight_dgrad_b16k), the masked
    dgrad of the 1x1 `confusion` (64 output channels) the streaming kernel of csrc/conv1x1_b16k.hip.  Yardstick:
    the same arithmetic in fp64 on the bf16-ROUNDED operands (dz, weights, stored activation, partial gradient) -- out = bf16 of
    (conv_transpose(dz, w) + res) where the stored activation's BatchNorm + ReLU was on: >= 99 % of the elements identical, the
    rest within one bf16 ulp (+ the fp32-accumulation floor next to zero); BatchNorm-backward sums sum(x), sum(x * xhat)
    over every slab entry within 1e-4 of the tensor's scale (they are taken from the fp32 values, not the rounded ones)."""
    from tactilesr_amd.model._train import conv_ex, Act, _pack_dgrad
    from tactilesr_amd._lib import load
    g = torch.Generator().manual_seed(ks * 7 + cin + cout + B)
    NP = 128 if cin % 128 == 0 else 64          # the launch's output slice: 128 channels, or 64 (the 64-channel layers)
    q = lambda t: t.bfloat16().float()
    dy = q(torch.randn(B, cout, H, W, generator=g))
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
    z = q(torch.randn(B, cin, H, W, generator=g))
    extra = q(torch.randn(B, cin, H, W, generator=g) * 0.1)
    msc, msh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    ba, bb = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    lib = load()
    to16 = lambda t, ctot=None, coff=0: T.to_cb16(t.cuda(), ctot, coff).to(torch.bfloat16)
    dyd, zd, exd = to16(dy), to16(z), to16(extra)
    gbuf = torch.full((B * cin * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
    entries = lib.tsr_conv2d_slab_entries_ex(B, H, W, NP, ks, -3)
    wd = w.cuda().contiguous()
    full = F.conv_transpose2d(dy.double(), q(w).double(), padding=ks // 2)
    for o in range(0, cin, NP):
        assert lib.tsr_conv2d_ex_dgrad_b16k(NP, cout, ks) == 1
        slab = torch.full((entries * NP * 2,), float("nan"), device="cuda")
        wp = _pack_dgrad(wd, cout, cin, ks, o, NP, -3)
        sl = slice(o, o + NP)
        mk = Act(zd, cin, o, NP, msc[sl].cuda().contiguous(), msh[sl].cuda().contiguous(), ba[sl].cuda().contiguous(),
                 bb[sl].cuda().contiguous())
        conv_ex(B=B, H=H, W=W, src=Act(dyd, cout, 0, cout), w=wp, cout=NP, ks=ks, out=gbuf, out_ctot=cin, out_coff=o,
                res=Act(exd, cin, o, NP) if res else None, epi_mode=2, mask=mk, bn=True, slab=slab, nsplit=-3)
        if o == 0 and ks > 1:   # the unmasked form (the first half of a two-conv gradient): out = bf16(conv_transpose(dz, w))
            g0 = torch.full((B * NP * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
            conv_ex(B=B, H=H, W=W, src=Act(dyd, cout, 0, cout), w=wp, cout=NP, ks=ks, out=g0, out_ctot=NP, out_coff=0, nsplit=-3)
            r0 = full[:, sl].float().bfloat16().float()
            d0 = (T.from_cb16(g0, B, NP, H, W).float().cpu() - r0).abs()
            assert float((d0 == 0).float().mean()) >= 0.99
            assert not (d0 > torch.maximum(1.01 * r0.abs() * 2.0 ** -7, torch.full_like(r0, 3e-6 * float(r0.abs().max())))).any()
        x = full[:, sl] + (extra[:, sl].double() if res else 0.0)
        on = (z[:, sl].double() * msc[sl].double().view(1, -1, 1, 1) + msh[sl].double().view(1, -1, 1, 1)) > 0
        x = torch.where(on, x, torch.zeros_like(x))
        ref = x.float().bfloat16().float()
        got = T.from_cb16(gbuf, B, cin, H, W)[:, sl].float().cpu()
        ulp = (ref.abs() * 2.0 ** -7).clamp_min(1e-30)
        d = (got - ref).abs()
        same = float((d == 0).float().mean())
        floor = 3e-6 * float(ref.abs().max())
        bad = d > torch.maximum(1.01 * ulp, torch.full_like(ulp, floor))
        xhat = z[:, sl].double() * ba[sl].double().view(1, -1, 1, 1) + bb[sl].double().view(1, -1, 1, 1)
        s1, s2 = x.sum(dim=(0, 2, 3)), (x * xhat).sum(dim=(0, 2, 3))
        sums = slab.view(entries, NP, 2).double().sum(0).cpu()
        e1 = float((sums[:, 0] - s1).abs().max() / s1.abs().max()), float((sums[:, 1] - s2).abs().max() / s2.abs().max())
        print(f"[b16k dgrad] k{ks} {cout}->{cin}[{o}:{o + NP}] B={B} {H}x{W}: identical {same:.5f}, beyond one ulp {int(bad.sum())}, "
              f"sums {e1[0]:.1e} / {e1[1]:.1e}")
        assert same >= 0.99 and not bad.any()
        assert e1[0] < 1e-4 and e1[1] < 1e-4
    assert not torch.isnan(gbuf.float()).any()


@pytest.mark.parametrize("ks,cin,B,H,W,cout", [(5, 128, 5, 16, 24, 128), (3, 128, 2, 40, 40, 128), (3, 256, 3, 13, 21, 128),
                                               (5, 64, 1, 5, 3, 128), (3, 64, 3, 13, 21, 64), (3, 512, 2, 40, 40, 64), (5, 64, 5, 16, 24, 64)])
def test_conv2d_train_forward_bf16_storage_b16k(T, ks, cin, B, H, W, cout):
    """Training with bf16 activation storage: the forward launches of the 128-output-channel 3x3 / 5x5 layers that feed a
    BatchNorm run csrc/conv_b16k.hip (tsr_conv2d_ex, nsplit = -3, epi_mode = 1; weights from tsr_pack_conv_weight_b16k) on a
    plain (materialised) bf16 input.  Yardstick: the convolution in fp64 on the bf16-ROUNDED operands -- out = bf16 of it
    (>= 99 % identical, the rest one ulp / the fp32-accumulation floor) and, merged over every slab entry (Chan), the
    per-channel mean / biased variance of the UNROUNDED output within 1e-5 of the tensor's scale; counts sum to B*H*W."""
    from tactilesr_amd.model._train import conv_ex, Act
    from tactilesr_amd._lib import load, call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(ks * 5 + cin + B + H)
    q = lambda t: t.bfloat16().float()
    x = q(torch.randn(B, cin, H, W, generator=g))
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
    lib = load()
    assert lib.tsr_conv2d_ex_dgrad_b16k(cout, cin, ks) == 1
    xd = T.to_cb16(x.cuda(), cin + 16, 16).to(torch.bfloat16)
    wp = torch.empty(lib.tsr_conv_weight_b16k_elems(cout, cin, ks), dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_conv_weight_b16k", ptr(w.cuda().contiguous()), ptr(wp), I(cout), I(cin), I(ks), stream())
    entries = lib.tsr_conv2d_slab_entries_ex(B, H, W, cout, ks, -1)
    slab = torch.full((entries * cout * 2,), float("nan"), device="cuda")
    cnt = torch.full((entries,), float("nan"), device="cuda")
    out = torch.full((B * (cout + 32) * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
    conv_ex(B=B, H=H, W=W, src=Act(xd, cin + 16, 16, cin), w=wp, cout=cout, ks=ks, out=out, out_ctot=cout + 32, out_coff=16,
            epi_mode=1, slab=slab, slab_cnt=cnt, nsplit=-3)
    ref = F.conv2d(x.double(), q(w).double(), padding=ks // 2)
    r16 = ref.float().bfloat16().float()
    got = T.from_cb16(out, B, cout + 32, H, W)[:, 16:16 + cout].float().cpu()
    d = (got - r16).abs()
    same = float((d == 0).float().mean())
    bad = d > torch.maximum(1.01 * r16.abs() * 2.0 ** -7, torch.full_like(r16, 3e-6 * float(r16.abs().max())))
    n_e = cnt.double().cpu()
    sl = slab.view(entries, cout, 2).double().cpu()
    N = float(n_e.sum())
    mean = (sl[:, :, 0] * n_e[:, None]).sum(0) / N
    m2 = (sl[:, :, 1] + n_e[:, None] * (sl[:, :, 0] - mean[None]) ** 2).sum(0)
    rm, rv = ref.mean(dim=(0, 2, 3)), ref.var(dim=(0, 2, 3), unbiased=False)
    e_m, e_v = float((mean - rm).abs().max() / ref.abs().max()), float((m2 / N - rv).abs().max() / rv.max())
    print(f"[b16k train fwd] k{ks} {cin}->{cout} B={B} {H}x{W}: identical {same:.5f}, beyond one ulp {int(bad.sum())}, "
          f"mean {e_m:.1e}, var {e_v:.1e}")
    assert N == B * H * W and same >= 0.99 and not bad.any()
    assert e_m < 1e-5 and e_v < 1e-5


@pytest.mark.parametrize("cin,B,H,W", [(64, 5, 16, 24), (64, 2, 40, 40), (96, 3, 13, 21)])
def test_conv2d_train_forward_pair_bf16_storage_b16k(T, cin, B, H, W):
    """The stage-1 pair of an MSRB in train mode with bf16 storage (tsr_conv2d_ex, nsplit = -4): conv_3_1 || conv_5_1 as one
    launch -- channels 0..63 = the 3x3 conv, 64..127 = the 5x5 conv of the same input, raw bf16 output + Welford partials.
    Yardstick as test_conv2d_train_forward_bf16_storage_b16k, each half against its own fp64 convolution."""
    from tactilesr_amd.model._train import conv_ex, Act
    from tactilesr_amd._lib import load, call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(cin + B + H)
    q = lambda t: t.bfloat16().float()
    x = q(torch.randn(B, cin, H, W, generator=g))
    w3, w5 = torch.randn(64, cin, 3, 3, generator=g) * 0.08, torch.randn(64, cin, 5, 5, generator=g) * 0.05
    lib = load()
    xd = T.to_cb16(x.cuda()).to(torch.bfloat16)
    w = torch.cat([F.pad(w3, (1, 1, 1, 1)), w5], 0).cuda().contiguous()
    wp = torch.empty(lib.tsr_conv_weight_b16k_pair_elems(cin), dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_conv_weight_b16k_pair", ptr(w), ptr(wp), I(cin), stream())
    entries = lib.tsr_conv2d_slab_entries_ex(B, H, W, 128, 5, -1)
    slab = torch.full((entries * 128 * 2,), float("nan"), device="cuda")
    cnt = torch.full((entries,), float("nan"), device="cuda")
    out = torch.full((B * 128 * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
    conv_ex(B=B, H=H, W=W, src=Act(xd, cin, 0, cin), w=wp, cout=128, ks=5, out=out, out_ctot=128, out_coff=0,
            epi_mode=1, slab=slab, slab_cnt=cnt, nsplit=-4)
    ref = torch.cat([F.conv2d(x.double(), q(w3).double(), padding=1), F.conv2d(x.double(), q(w5).double(), padding=2)], 1)
    r16 = ref.float().bfloat16().float()
    got = T.from_cb16(out, B, 128, H, W).float().cpu()
    d = (got - r16).abs()
    same = float((d == 0).float().mean())
    bad = d > torch.maximum(1.01 * r16.abs() * 2.0 ** -7, torch.full_like(r16, 3e-6 * float(r16.abs().max())))
    n_e = cnt.double().cpu()
    sl = slab.view(entries, 128, 2).double().cpu()
    N = float(n_e.sum())
    mean = (sl[:, :, 0] * n_e[:, None]).sum(0) / N
    m2 = (sl[:, :, 1] + n_e[:, None] * (sl[:, :, 0] - mean[None]) ** 2).sum(0)
    rm, rv = ref.mean(dim=(0, 2, 3)), ref.var(dim=(0, 2, 3), unbiased=False)
    e_m, e_v = float((mean - rm).abs().max() / ref.abs().max()), float(((m2 / N - rv).abs() / rv).max())
    print(f"[b16k train pair] {cin}->64|64 B={B} {H}x{W}: identical {same:.5f}, beyond one ulp {int(bad.sum())}, "
          f"mean {e_m:.1e}, var {e_v:.1e}")
    assert N == B * H * W and same >= 0.99 and not bad.any()
    assert e_m < 1e-5 and e_v < 1e-5


@pytest.mark.parametrize("cin,B,H,W,relu,res", [(256, 3, 13, 21, 1, True), (256, 2, 40, 40, 1, "virtual"), (128, 70, 12, 12, 0, False),
                                               (256, 1, 5, 3, 1, True)])
def test_conv1x1_forward_virtual_input_bf16_storage_b16k(T, cin, B, H, W, relu, res):
    """The forward of the MSRB's 1x1 `confusion` with bf16 storage (tsr_conv2d_ex, nsplit = -3, ks = 1, epi_mode 0;
    csrc/conv1x1_b16k.hip): the input is VIRTUAL -- relu(z * in_scale + in_shift) of the stored bf16 z, formed in LDS behind the
    DMA, rounded to bf16 like the register-staging kernels do -- the weight bf16, bias + residual + ReLU in the epilogue.
    Yardstick: the same arithmetic in fp64 on the bf16-ROUNDED operands; >= 99 % of the outputs identical, the rest within
    one bf16 ulp (+ the fp32-accumulation floor).  Ragged pixel counts, a C_in of 128, with / without residual and ReLU."""
    from tactilesr_amd.model._train import conv_ex, Act
    from tactilesr_amd._lib import load, call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(cin + B + H)
    q = lambda t: t.bfloat16().float()
    z = q(torch.randn(B, cin, H, W, generator=g))
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    w = torch.randn(64, cin, 1, 1, generator=g) * 0.08
    bias = torch.randn(64, generator=g) * 0.1
    r = q(torch.randn(B, 64, H, W, generator=g))
    lib = load()
    assert lib.tsr_conv2d_ex_fwd1x1_b16k(64, cin) == 1
    a = q(F.relu(torch.addcmul(sh.view(1, -1, 1, 1), z, sc.view(1, -1, 1, 1))))
    rsc, rsh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    rterm = 0.0
    if res == "virtual":        # the first MSRB's residual: relu(r * scale + shift) of a stored pre-BatchNorm tensor (fp32, not rounded)
        rterm = F.relu(torch.addcmul(rsh.view(1, -1, 1, 1), r, rsc.view(1, -1, 1, 1))).double()
    elif res:
        rterm = r.double()
    ref = F.conv2d(a.double(), q(w).double()) + bias.double().view(1, -1, 1, 1) + rterm
    ref = F.relu(ref) if relu else ref
    r16 = ref.float().bfloat16().float()
    zd = T.to_cb16(z.cuda(), cin + 16, 16).to(torch.bfloat16)
    rd = T.to_cb16(r.cuda(), 96, 32).to(torch.bfloat16)
    wp = torch.empty(lib.tsr_conv_weight_b16k_elems(64, cin, 1), dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_conv_weight_b16k", ptr(w.cuda().contiguous()), ptr(wp), I(64), I(cin), I(1), stream())
    out = torch.full((B * 80 * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
    conv_ex(B=B, H=H, W=W, src=Act(zd, cin + 16, 16, cin, sc.cuda(), sh.cuda()), w=wp, cout=64, ks=1, out=out, out_ctot=80,
            out_coff=16, shift=bias.cuda(), relu=relu,
            res=(Act(rd, 96, 32, 64, rsc.cuda(), rsh.cuda()) if res == "virtual" else Act(rd, 96, 32, 64)) if res else None, nsplit=-3)
    full = T.from_cb16(out, B, 80, H, W).float().cpu()
    got = full[:, 16:80]
    d = (got - r16).abs()
    same = float((d == 0).float().mean())
    bad = d > torch.maximum(1.01 * r16.abs() * 2.0 ** -7, torch.full_like(r16, 3e-6 * float(r16.abs().max())))
    print(f"[b16k 1x1 fwd] {cin}->64 B={B} {H}x{W}: identical {same:.5f}, beyond one ulp {int(bad.sum())}")
    assert same >= 0.99 and not bad.any()
    assert torch.isnan(full[:, :16]).all()          # outside the slice: untouched


def _subs(t, k=512):
    t = t.detach().flatten()
    return t[:: max(1, t.numel() // k)].cpu().numpy()


@pytest.mark.parametrize("impl", ["bf16x6", "fp16x3", "f32"])
def test_train_forward_backward_vs_reference_golden(T, golden, impl):
    g = golden("train")
    cfg = dict(patternFeatureExtraLayerCnt=2)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), int(g["seed"]))
    m = T.TactileSR(**cfg)
    m.train_impl = impl            # explicit arithmetic choice (no environment switch)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    _debug_engine(m)
    LR, HR = torch.from_numpy(g["LR"]).cuda(), torch.from_numpy(g["HR_prepared"]).cuda()
    out = m(LR[:, :3])
    assert relerr(out, torch.from_numpy(g["out0"])) < 1e-5
    loss = torch.nn.MSELoss()(out, HR)
    assert abs(loss.item() - g["losses"][0]) <= 1e-5 * abs(g["losses"][0])
    loss.backward()
    named = dict(m.named_parameters())
    # Gradients, hard bar: max-norm 1e-5 on EVERY parameter against the fp64 oracle gradient evaluated on the ReLU
    # pattern the device took; the pattern itself must equal the fp64 pattern except at pre-activations that are
    # zero to rounding (tests/_gradcheck.py explains why the two halves are separated).
    masks = {k: v.cpu() for k, v in m._train_engine.activation_masks(m._train_engine.last_ctx).items()}
    LRc, HRc = torch.from_numpy(g["LR"])[:, :3], torch.from_numpy(g["HR_prepared"])
    l64, _, _, pre64 = GC.oracle_grads(sd, LRc, HRc, record=True)
    assert abs(l64 - float(g["loss64"])) <= 1e-9 * abs(l64)          # the oracle's fp64 run IS the reference's
    flips = GC.check_pattern(masks, pre64)
    _, g64m, _, _ = GC.oracle_grads(sd, LRc, HRc, masks=masks)
    worst = GC.check_grads({k: p.grad for k, p in named.items()}, g64m, tol=1e-5)
    print(f"[grad {impl}] {flips} ReLU flips vs fp64; worst on-pattern max-norm error {worst[0]:.2e} ({worst[1]})")
    # Gradients, bridge to the reference's own numbers: the fixture holds the reference's fp32 and fp64 gradients
    # (each on its own ReLU pattern).  The HIP gradient must sit as close to the reference's fp64 run as the
    # reference's fp32 run does (x4: the flip sets are independent draws), in max-norm AND in relative L2.
    for k in [str(k) for k in g["keys"]]:
        gk = named[k].grad
        assert gk is not None, k
        ref32, ref64 = g[f"grad/{k}"].astype(np.float64), g[f"grad64/{k}"]
        got = _subs(gk).astype(np.float64)
        den = max(np.abs(ref64).max(), 1e-30)
        if float(g[f"gradnorm/{k}"]) < 1e-4:      # conv bias in front of a train-mode BN: gradient == 0 + noise
            assert np.abs(got).max() < 1e-4, k
            continue
        e_hip, e_ref = np.abs(got - ref64).max() / den, np.abs(ref32 - ref64).max() / den
        n64 = max(np.linalg.norm(ref64), 1e-30)
        l2_hip, l2_ref = float(np.linalg.norm(got - ref64) / n64), float(np.linalg.norm(ref32 - ref64) / n64)
        print(f"[grad] {k}: hip-vs-f64 {e_hip:.2e} (L2 {l2_hip:.2e})  ref32-vs-f64 {e_ref:.2e} (L2 {l2_ref:.2e})")
        assert e_hip <= max(1e-5, 4 * e_ref) and l2_hip <= max(1e-5, 4 * l2_ref), (k, e_hip, e_ref, l2_hip, l2_ref)
    new_sd = m.state_dict()
    for s in [str(s) for s in g["stat_keys"]]:
        assert relerr(new_sd[s + ".running_mean"], torch.from_numpy(g[f"stat/{s}.running_mean"])) < 1e-5, s
        assert relerr(new_sd[s + ".running_var"], torch.from_numpy(g[f"stat/{s}.running_var"])) < 1e-5, s
        assert int(new_sd[s + ".num_batches_tracked"]) == int(g[f"stat/{s}.num_batches_tracked"])
    # every parameter received a gradient
    assert all(p.grad is not None for p in m.parameters())


@pytest.mark.parametrize("impl", ["bf16x6", "fp16x3"])
def test_full_step_adam_vs_reference_golden(T, golden, impl):
    """train_cal_loss + zero_grad/backward/Adam(L2) step through the HIP path, twice; post-step weights,
    running stats and the second-step loss vs the reference's own run."""
    from tactilesr_amd import optim
    from tactilesr_amd.train import tactileSR_train as TR
    g = golden("train")
    cfg = dict(patternFeatureExtraLayerCnt=2)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), int(g["seed"]))
    m = T.TactileSR(**cfg)
    m.train_impl = impl            # explicit arithmetic choice (no environment switch)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    conf = TR.default_config()
    batch = (torch.from_numpy(g["LR"]), torch.from_numpy(g["HR_raw"]))
    l0 = TR.train_one_iter(m, opt, batch, conf)["total_loss"].item()
    assert abs(l0 - g["losses"][0]) <= 1e-5 * abs(g["losses"][0])
    new_sd = m.state_dict()
    for k in [str(k) for k in g["keys"]]:
        w = new_sd[k]
        # Adam's first step moves every weight by lr*g'/(|g'|+eps), g' = g + wd*w: the step is +-lr whatever |g'| is,
        # so a weight can differ from the reference's only where the SIGN of g' differs, i.e. where |g'| is below
        # the gradient's ReLU-flip noise floor (~1e-3 of its max, see test_train_forward_backward...).  Every probe
        # that differs must be such a near-zero-gradient probe, must differ by at most 2*lr, and they must be few.
        diff = np.abs(_subs(w) - g[f"w1/{k}"])
        off = diff > 1e-6 + 1e-5 * np.abs(g[f"w1/{k}"])
        gp = g[f"grad/{k}"].astype(np.float64) + 1e-2 * _subs(sd[k]).astype(np.float64)
        assert diff.max() <= 2.1e-3 and off.mean() < 0.02, (k, diff.max(), off.mean())
        if off.any():
            assert np.abs(gp[off]).max() < 3e-3 * np.abs(gp).max(), (k, np.abs(gp[off]).max(), np.abs(gp).max())
    l1 = TR.train_one_iter(m, opt, batch, conf)["total_loss"].item()
    assert abs(l1 - g["losses"][1]) <= 2e-4 * abs(g["losses"][1])
    assert int(opt.state[next(iter(m.parameters()))]["step"]) == 2


def test_target_prep_mse_and_metrics(T, golden):
    from tactilesr_amd import functional as Fh
    g = golden("train")
    HR = Fh.prepare_target(torch.from_numpy(g["HR_raw"]).cuda(), 10.0, 10)
    assert relerr(HR, torch.from_numpy(g["HR_prepared"])) < 1e-6
    gm = golden("metrics")
    a, b = torch.from_numpy(gm["a"]).cuda(), torch.from_numpy(gm["b"]).cuda()
    ps, ss = Fh.psnr_ssim(a, b, 250.0, reference_quirk=True)
    assert np.abs(ps.cpu().numpy() - gm["psnr_140"]).max() < 1e-3
    assert np.abs(ss.cpu().numpy() - gm["ssim_140"]).max() < 1e-6
    ps2, _ = Fh.psnr_ssim(a, b, 250.0, reference_quirk=False)
    assert np.abs(ps2.cpu().numpy() - gm["psnr_40"]).max() < 1e-3
    y = a.clone().requires_grad_(True)
    loss = Fh.mse_loss(y, b)
    ref = torch.nn.functional.mse_loss(a.cpu(), b.cpu())
    assert abs(loss.item() - ref.item()) < 1e-6 * ref.item()
    loss.backward()
    assert relerr(y.grad, 2 * (a - b).cpu() / a.numel()) < 1e-6


def test_eval_func_after_training_uses_updated_running_stats(T):
    """eval after a train step must see the running statistics the kernels updated in place."""
    from tactilesr_amd import optim
    from tactilesr_amd.train import tactileSR_train as TR
    torch.manual_seed(3)
    m = T.TactileSR(patternFeatureExtraLayerCnt=1).cuda()
    conf = TR.default_config()
    g = torch.Generator().manual_seed(5)
    batch = (torch.rand(6, 3, 4, 4, generator=g) * 8, torch.rand(6, 1, 100, 100, generator=g) * 250)
    m.eval()
    y0 = m(batch[0].cuda())
    m.train()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    TR.train_one_iter(m, opt, batch, conf)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    loss, ssim, psnr = TR.eval_func(m, [batch], conf)
    with torch.no_grad():
        ref_mse, ref_psnr, ref_ssim = O.eval_batch(sd, batch[0], batch[1], 250.0)
    assert abs(loss - ref_mse) < 1e-4 * ref_mse
    assert abs(psnr - ref_psnr) < 1e-2 and abs(ssim - ref_ssim) < 1e-4
    assert not torch.equal(m(batch[0].cuda()), y0)


@pytest.mark.parametrize("Tn,nm,B,sf", [(2, 1, 3, 10), (2, 1, 4, 10), (1, 2, 3, 10), (1, 1, 2, 25), (2, 1, 1, 25)])
def test_train_multiframe_and_odd_batch_vs_oracle(T, Tn, nm, B, sf):
    """seqsCnt=2 (two stems -> channel-stacked fuse conv) and odd batches (image-pair tail): loss, running stats
    and EVERY parameter gradient against the CPU oracle in fp64, max-norm 1e-5 on the device's own ReLU pattern
    (tests/_gradcheck.py); the pattern may differ from fp64's only at pre-activations that are zero to rounding.
    sf=25 is the tactileSRSeqs output size: 100x100 = 12.5 patches of 8 (ragged tiles in every train-mode epilogue,
    dgrad and wgrad)."""
    _train_step_vs_oracle(T, dict(seqsCnt=Tn, patternFeatureExtraLayerCnt=nm, scale_factor=sf), B, 977)


def _train_step_vs_oracle(T, cfg, B, seed, tol=1e-5, loss_tol=1e-5):
    return GC.train_step_vs_oracle(T, cfg, B, seed, tol=tol, loss_tol=loss_tol)[0]


def test_train_step_distinct_frames_wide_amplitude_vs_oracle(T):
    """The train step on 160 DISTINCT frames whose taxel amplitudes span 2^8 (frame k: rand * 8 * 2^-(k mod 9)) -- the
    large-batch train tests tile 32 frames, and every operand scale of the fp16x3 path (activations, dz, gradients) is a
    tensor-wide max|.|, so quiet frames share their scales with frames 256x louder in forward AND backward.  Loss and
    running statistics at 1e-5, the ReLU pattern equal to fp64's up to rounding-zero flips, every parameter gradient at
    1e-5 (max-norm) against the fp64 oracle gradient on the device's pattern; and the OUTPUT per frame relative to the
    frame's own maximum, quiet classes at 1e-5 (train-mode BatchNorm couples the frames through the batch statistics,
    so a quiet frame's activations are not small -- the check is on what the tensor-wide scale does to them)."""
    cfg = dict(patternFeatureExtraLayerCnt=2)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), 4711)
    g = torch.Generator().manual_seed(4712)
    B = 160
    cls = torch.arange(B) % 9
    LR = torch.rand(B, 3, 4, 4, generator=g) * 8 * (2.0 ** -cls.float()).view(-1, 1, 1, 1)
    HR = torch.rand(B, 1, 40, 40, generator=g) * 25
    l64, _, ns64, pre64 = GC.oracle_grads(sd, LR, HR, record=True)
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    eng = _debug_engine(m)
    out = m(LR.cuda())
    loss = F.mse_loss(out, HR.cuda())
    assert abs(loss.item() - l64) < 1e-5 * abs(l64)
    with torch.no_grad():
        ref = O.tactilesr_forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, LR.double(),
                                  training=True)
    per = (out.detach().cpu().double() - ref).abs().amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3)).clamp_min(1e-30)
    live = ref.abs().amax(dim=(1, 2, 3)) > 1e-3 * float(ref.abs().max())
    quiet = live & (cls >= 5)
    print(f"[train wide amplitude] per-frame output error: quiet classes {float(per[quiet].max()):.2e}, all live frames "
          f"{float(per[live].max()):.2e}")
    assert int(quiet.sum()) >= 60 and float(per[quiet].max()) < 1e-5
    loss.backward()
    new_sd = m.state_dict()
    for k, v in ns64.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert relerr(new_sd[k], v) < 1e-5, k
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    flips = GC.check_pattern(masks, pre64)
    _, g64m, _, _ = GC.oracle_grads(sd, LR, HR, masks=masks)
    worst = GC.check_grads({k: p.grad for k, p in m.named_parameters()}, g64m, tol=1e-5)
    print(f"[train wide amplitude] {flips} ReLU flips; worst on-pattern grad error {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("B", [1, 2])
def test_train_step_seqs_T8_sf25_vs_oracle(T, B):
    """BASELINE configs[4] shape as a TRAIN step: TactileSR(scale_factor=25, seqsCnt=8), 4x4x24 -> 100x100, default
    fp16x3 arithmetic against the fp64 oracle (2 MSRBs keep the CPU side in seconds; every kernel shape of the full
    net is exercised: 8 stems, the 512->64 fuse conv, ragged 12.5-patch tiles).  Gradient bar 2e-5 (the sf = 10 tests hold
    1e-5): 10^4 output pixels funnel into 16 LR taxels per stem weight; measured 1.07e-5 on ONE stem weight tensor."""
    _train_step_vs_oracle(T, dict(seqsCnt=8, scale_factor=25, patternFeatureExtraLayerCnt=2), B, 1977, tol=2e-5)


def test_train_step_seqs_T8_sf25_bf16_reduced_precision(T):
    """configs[4] as BASELINE words it ("bf16"): plain bf16 conv operands, fp32 accumulate/parameters.  Not the
    parity path; bar 2e-2 on the loss and cosine > 0.95 per gradient tensor against fp64."""
    cfg = dict(seqsCnt=8, scale_factor=25, patternFeatureExtraLayerCnt=2)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), 1977)
    g = torch.Generator().manual_seed(1978)
    LR = torch.rand(2, 24, 4, 4, generator=g) * 8
    HR = torch.rand(2, 1, 100, 100, generator=g) * 25
    l64, g64, _, _ = GC.oracle_grads(sd, LR, HR, scale_factor=25)
    m = T.TactileSR(**cfg)
    m.train_impl = "bf16"            # explicit arithmetic choice (no environment switch)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    loss = F.mse_loss(m(LR.cuda()), HR.cuda())
    assert abs(loss.item() - l64) < 2e-2 * abs(l64)
    loss.backward()
    for k, p in m.named_parameters():
        ref = g64[k]
        if float(ref.abs().max()) < 1e-6:
            continue
        got = p.grad.detach().cpu().double().flatten()
        cos = float(got @ ref.flatten() / (got.norm() * ref.norm()).clamp_min(1e-30))
        assert cos > 0.95, (k, cos)      # measured worst 0.978 (a stem weight: 8 plain-bf16 stems feed a 512-ch fuse conv)


def _tiled_train_step(T, reps, cfg, seed, tol=1e-5, base=32):
    """Size-independent property at a large batch (`base` frames tiled `reps` times): batch statistics, the MSE
    loss and hence every gradient of a tiled batch equal those of the base frames, which the CPU oracle can run.
    The activation pattern of the first `base` frames must equal fp64's up to rounding-zero flips, all replicas must
    carry the SAME pattern, and every gradient meets the max-norm bar on that pattern."""
    sf, Tn = cfg.get("scale_factor", 10), cfg.get("seqsCnt", 1)
    torch.manual_seed(seed)
    m = T.TactileSR(**cfg)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    LRb, HRb = torch.rand(base, 3 * Tn, 4, 4, generator=g) * 8, torch.rand(base, 1, 4 * sf, 4 * sf, generator=g) * 25
    m = m.cuda().train()
    eng = _debug_engine(m)
    out = m(LRb.repeat(reps, 1, 1, 1).cuda())
    loss = F.mse_loss(out, HRb.repeat(reps, 1, 1, 1).cuda())
    loss.backward()
    torch.cuda.synchronize()
    l64, _, _, pre64 = GC.oracle_grads(sd, LRb, HRb, scale_factor=sf, record=True)
    assert abs(loss.item() - l64) < 1e-5 * l64
    o = out.view(reps, base, -1)
    assert torch.equal(o, o[:1].expand_as(o))                 # replicas are bit-identical in train mode too
    ctx = eng.last_ctx
    masks = {k: v.cpu() for k, v in eng.activation_masks(ctx, 0, base).items()}
    for k, v in eng.activation_masks(ctx, base * (reps - 1), base).items():      # last replica: same pattern
        assert torch.equal(v.cpu(), masks[k]), k
    del ctx
    eng.last_ctx = None
    flips = GC.check_pattern(masks, pre64)
    _, g64m, _, _ = GC.oracle_grads(sd, LRb, HRb, scale_factor=sf, masks=masks)
    worst = GC.check_grads({k: p.grad for k, p in m.named_parameters()}, g64m, tol=tol)
    print(f"[tiled {base} x{reps} {cfg}] {flips} ReLU flips; worst on-pattern grad error {worst[0]:.2e} ({worst[1]})")
    return m


def test_large_batch_train_step_tiling_invariance(T):
    _tiled_train_step(T, 32, dict(patternFeatureExtraLayerCnt=2), 5)


def test_train_step_B8192_tiling_invariance(T):
    """BASELINE configs[2]/[3] per-GPU batch: one full TactileSR (6 MSRB) train step at B = 8192 (168 GB of saved
    activations in HBM) = 32 frames x 256.  Gradient bar 2e-5 here (every other whole-step test: 1e-5): a weight-gradient
    entry is an fp32 sum of 8192 x 1600 products; measured 1.2e-5 of the tensor max on four conv_5_2 weights (the
    same step at 32 x 5 frames holds 1e-5)."""
    torch.cuda.empty_cache()
    m = _tiled_train_step(T, 256, dict(), 42, tol=2e-5)
    del m
    torch.cuda.empty_cache()


def test_seqs_train_step_B256_full_size_tiling_invariance(T):
    """BASELINE configs[4] at the size bench.py's `seqs_train_b256` leg runs: the FULL TactileSR(scale_factor=25,
    seqsCnt=8) (6 MSRBs, 100x100 output) train step at B = 256 = 2 base frame-stacks x 128.  Replicas bit-identical,
    loss 1e-5 against the fp64 oracle on the base frames, the ReLU pattern fp64's up to rounding-zero flips and the same
    in the last replica, every parameter gradient on that pattern within 2e-5 (the bar of the small Seqs test)."""
    torch.cuda.empty_cache()
    m = _tiled_train_step(T, 128, dict(scale_factor=25, seqsCnt=8), 4242, tol=2e-5, base=2)
    del m
    torch.cuda.empty_cache()


def test_seqs_eval_B512_full_size_tiling_invariance(T):
    """... and the `seqs_eval_b512` leg's size: eval forward of the full sf = 25 / T = 8 model at B = 512 = 4 distinct
    frame-stacks x 128, trained-like BatchNorm statistics.  Frames are independent in eval mode: every replica is
    bit-identical to the first, and the 4 distinct outputs meet 1e-5 against the CPU oracle."""
    cfg = dict(scale_factor=25, seqsCnt=8)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), 5125)
    g = torch.Generator().manual_seed(5126)
    LRb = torch.rand(4, 24, 4, 4, generator=g) * 8
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    with torch.no_grad():
        out = m(LRb.repeat(128, 1, 1, 1).cuda())
        ref = O.tactilesr_forward(sd, LRb, scale_factor=25)
    assert out.shape == (512, 1, 100, 100)
    o = out.view(128, 4, -1)
    assert torch.equal(o, o[:1].expand_as(o))
    e = relerr(out[:4], ref)
    print(f"[seqs eval B=512] base frames vs oracle {e:.2e}")
    assert e < 1e-5


def test_bf16_storage_train_step_B8192_full_size_tiling_invariance(T):
    """BASELINE configs[2] at the size bench.py's `train_bf16_b8192` leg runs: the full 6-MSRB model, every activation /
    gradient tensor stored as bf16 CB16, B = 8192 = 32 frames x 256 (84 GB of saved tensors).  Replicas bit-identical;
    loss within 2e-3 of the bf16-EMULATING oracle's loss on the 32 base frames (the yardstick of every bf16 test: the
    reference has no bf16 numerics); every parameter gradient pointing the emulated one's way (cosine >= 0.995) with the
    norm within 5 %; running statistics within 2e-3."""
    torch.cuda.empty_cache()
    torch.manual_seed(42)
    m = T.TactileSR()
    m.train_impl = "bf16"            # explicit arithmetic choice (no environment switch)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(43)
    LRb, HRb = torch.rand(32, 3, 4, 4, generator=g) * 8, torch.rand(32, 1, 40, 40, generator=g) * 25
    m = m.cuda().train()
    out = m(LRb.repeat(256, 1, 1, 1).cuda())
    assert m.train_engine().io16
    loss = F.mse_loss(out, HRb.repeat(256, 1, 1, 1).cuda())
    loss.backward()
    o = out.view(256, 32, -1)
    assert torch.equal(o, o[:1].expand_as(o))
    l_e, g_e, ns_e, _ = _emulated_step(sd, LRb, HRb)
    assert abs(loss.item() - l_e) <= 2e-3 * abs(l_e), (loss.item(), l_e)
    new_sd = m.state_dict()
    for k, v in ns_e.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert relerr(new_sd[k], v) < 2e-3, k
    worst = 1.0
    gmax = float(max(v.abs().max() for v in g_e.values()))
    for k, p in m.named_parameters():
        ref = g_e[k].double().flatten()
        if float(ref.abs().max()) < 1e-6 * gmax:
            continue
        got = p.grad.detach().cpu().double().flatten()
        cos = float(got @ ref / (got.norm() * ref.norm()).clamp_min(1e-30))
        worst = min(worst, cos)
        assert cos >= 0.995, (k, cos)
        assert abs(float(got.norm() / ref.norm()) - 1.0) < 5e-2, (k, float(got.norm() / ref.norm()))
    print(f"[bf16-storage train B=8192] loss {abs(loss.item() - l_e) / abs(l_e):.2e} from the emulated loss, worst gradient "
          f"cosine {worst:.5f}")
    del m, out, loss
    torch.cuda.empty_cache()


def test_bf16_train_mode_is_a_reduced_precision_of_the_same_step(T, golden):
    """TSR_TRAIN_IMPL=bf16 (BASELINE's "bf16" configurations: bf16 conv operands, fp32 accumulation, parameters and
    activations) is NOT the parity path; it must still be the same computation: loss within 2e-2 of the reference's,
    every gradient pointing the same way (cosine > 0.98 against the fp64 yardstick)."""
    g = golden("train")
    cfg = dict(patternFeatureExtraLayerCnt=2)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), int(g["seed"]))
    m = T.TactileSR(**cfg)
    m.train_impl = "bf16"            # explicit arithmetic choice (no environment switch)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    LR, HR = torch.from_numpy(g["LR"]).cuda(), torch.from_numpy(g["HR_prepared"]).cuda()
    out = m(LR[:, :3])
    assert relerr(out, torch.from_numpy(g["out0"])) < 3e-2
    loss = torch.nn.MSELoss()(out, HR)
    assert abs(loss.item() - g["losses"][0]) <= 2e-2 * abs(g["losses"][0])
    loss.backward()
    named = dict(m.named_parameters())
    for k in [str(k) for k in g["keys"]]:
        if float(g[f"gradnorm/{k}"]) < 1e-4:
            continue
        got, ref = _subs(named[k].grad).astype(np.float64), g[f"grad64/{k}"]
        cos = float(got @ ref / max(np.linalg.norm(got) * np.linalg.norm(ref), 1e-30))
        assert cos > 0.98, (k, cos)


def test_seqs_bf16_storage_train_step_B256_full_size_tiling_invariance(T):
    """BASELINE configs[4] as worded ("tactileSRSeqs (T=8) 4x4 -> 100x100, bf16") at the size bench.py's `seqs_train_bf16_b256`
    leg runs: the full sf = 25 / T = 8 model (6 MSRBs), bf16 activation / gradient storage, B = 256 = 2 base frame-stacks x
    128.  Replicas bit-identical; loss within 2e-3 of the bf16-EMULATING oracle's on the 2 base stacks; every parameter gradient
    pointing the emulated one's way (cosine >= 0.99: eight plain-bf16 stems feed a 512-channel fuse conv, the small Seqs
    reduced-precision test measures 0.978 against fp64 there) with the norm within 5 %."""
    torch.cuda.empty_cache()
    cfg = dict(scale_factor=25, seqsCnt=8)
    torch.manual_seed(4242)
    m = T.TactileSR(**cfg)
    m.train_impl = "bf16"
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(4243)
    LRb, HRb = torch.rand(2, 24, 4, 4, generator=g) * 8, torch.rand(2, 1, 100, 100, generator=g) * 25
    m = m.cuda().train()
    out = m(LRb.repeat(128, 1, 1, 1).cuda())
    assert m.train_engine().io16
    loss = F.mse_loss(out, HRb.repeat(128, 1, 1, 1).cuda())
    loss.backward()
    o = out.view(128, 2, -1)
    assert torch.equal(o, o[:1].expand_as(o))
    l_e, g_e, _, _ = _emulated_step(sd, LRb, HRb, scale_factor=25)
    assert abs(loss.item() - l_e) <= 2e-3 * abs(l_e), (loss.item(), l_e)
    worst = 1.0
    gmax = float(max(v.abs().max() for v in g_e.values()))
    for k, p in m.named_parameters():
        ref = g_e[k].double().flatten()
        if float(ref.abs().max()) < 1e-6 * gmax:
            continue
        got = p.grad.detach().cpu().double().flatten()
        cos = float(got @ ref / (got.norm() * ref.norm()).clamp_min(1e-30))
        worst = min(worst, cos)
        assert cos >= 0.99, (k, cos)
        assert abs(float(got.norm() / ref.norm()) - 1.0) < 5e-2, (k, float(got.norm() / ref.norm()))
    print(f"[Seqs bf16-storage train B=256] loss {abs(loss.item() - l_e) / abs(l_e):.2e} from the emulated loss, worst gradient "
          f"cosine {worst:.5f}")
    del m, out, loss
    torch.cuda.empty_cache()


_emulated_step = GC.emulated_step


@pytest.mark.parametrize("cfg,B,seed", [(dict(patternFeatureExtraLayerCnt=2), 4, 211),
                                        (dict(seqsCnt=2, patternFeatureExtraLayerCnt=1), 11, 977),
                                        (dict(seqsCnt=8, scale_factor=25, patternFeatureExtraLayerCnt=1), 2, 1977)])
def test_train_step_bf16_storage_vs_bf16_emulating_oracle(T, cfg, B, seed):
    """TSR_TRAIN_IMPL=bf16 -- BASELINE's "bf16" train configurations: every stored activation / gradient tensor is bf16
    CB16 (saved pre-activations z, dz, dgrad outputs), bf16 MFMA operands, fp32 accumulation, fp32 master weights /
    BatchNorm statistics / weight gradients -- against the oracle's restatement of THAT arithmetic in the forward pass
    (bf16 rounding of every stored tensor and of the conv weights, statistics from the fp32 accumulator, fp32 epilogues;
    the reference has no bf16 numerics): loss within 2e-3, output max-norm within 2^-6 (two bf16 evaluations decorrelate
    to about one ulp RMS, see the eval test), running statistics within 2e-3, every parameter gradient pointing the same way as the
    emulated one (cosine >= 0.995; the oracle's backward keeps fp32 gradient tensors, the device rounds them to bf16).
    The two-stem case runs at B = 11 (odd: the image-group tail stays covered).  At B = 3, where it ran before the 64-channel
    layers moved to the LDS-DMA kernels, the worst cosine -- always a stem BatchNorm parameter -- is a property of the SEED, not
    of the kernels: seeds 977 / 978 / 979 give 0.9946 / 0.9981 / 0.9690 on the LDS-DMA kernels and 0.9961 / 0.9980 / 0.9642 on the
    32x32x16 kernels they replaced (tools/bf16_grad_cosine_probe.py); at B = 11: 0.9982 / 0.9991 / 0.9877 against 0.9985 /
    0.9990 / 0.9852."""
    GC.bf16_train_step_vs_emulating_oracle(T, cfg, B, seed)


def test_bf16_storage_train_step_tiling_invariance(T):
    """Larger batch through the bf16-storage train path (B = 512 = 32 frames x 16): replicas bit-identical, loss equal to
    the oracle's emulated loss on the 32 base frames within 2e-3."""
    torch.manual_seed(5)
    m = T.TactileSR(patternFeatureExtraLayerCnt=2)
    m.train_impl = "bf16"            # explicit arithmetic choice (no environment switch)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    LRb, HRb = torch.rand(32, 3, 4, 4, generator=g) * 8, torch.rand(32, 1, 40, 40, generator=g) * 25
    m = m.cuda().train()
    out = m(LRb.repeat(16, 1, 1, 1).cuda())
    loss = F.mse_loss(out, HRb.repeat(16, 1, 1, 1).cuda())
    loss.backward()
    o = out.view(16, 32, -1)
    assert torch.equal(o, o[:1].expand_as(o))
    l_e, g_e, _, _ = _emulated_step(sd, LRb, HRb)
    assert abs(loss.item() - l_e) <= 2e-3 * abs(l_e)
    k = "patternFeatureExtra_layer.1.conv_5_2.0.weight"
    got, ref = dict(m.named_parameters())[k].grad.cpu().double().flatten(), g_e[k].double().flatten()
    assert float(got @ ref / (got.norm() * ref.norm())) >= 0.995


def test_non_finite_loss_raises_like_the_reference_trainer(T):
    """cpu/trainer.py:280-284: a NaN / Inf loss raises FloatingPointError.  A NaN taxel, an Inf taxel and a diverged (NaN)
    weight must each reach the loss through the train-mode path (batch statistics couple every frame, so the whole
    batch goes non-finite -- as in the reference); `train_one_iter(check_finite=True)` raises with the reference's text."""
    from tactilesr_amd import optim
    from tactilesr_amd.train import tactileSR_train as TR
    conf = TR.default_config()
    g = torch.Generator().manual_seed(5)
    LR, HR = torch.rand(6, 3, 4, 4, generator=g) * 8, torch.rand(6, 1, 100, 100, generator=g) * 250
    for case in ("nan_taxel", "inf_taxel", "nan_weight"):
        torch.manual_seed(3)
        m = T.TactileSR(patternFeatureExtraLayerCnt=1).cuda().train()
        opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
        assert torch.isfinite(TR.train_one_iter(m, opt, (LR, HR), conf, check_finite=True, cur_iter=0)["total_loss"])
        bad = LR.clone()
        if case == "nan_taxel":
            bad[3, 1, 2, 2] = float("nan")
        elif case == "inf_taxel":
            bad[0, 2, 0, 3] = float("inf")
        else:
            with torch.no_grad():
                m.patternFeatureExtra_layer[0].conv_5_2[0].weight[7, 3, 2, 2] = float("nan")
        with pytest.raises(FloatingPointError, match="Loss became infinite or NaN at iteration=1"):
            TR.train_one_iter(m, opt, (bad, HR), conf, check_finite=True, cur_iter=1)


def test_multi_step_loss_trajectory_tracks_the_oracle(T):
    """Ten Adam(L2) steps on a fixed batch: the loss curve of the HIP path follows the CPU oracle's step by step.
    Two faithful fp32 implementations drift apart slowly (ReLU-mask flips, Adam's sign sensitivity near zero
    gradients): measured 3e-7 after one step, 5e-5 after ten; bars 2e-5 for the first three steps, 1e-3 throughout.
    (lr = 3e-5: at the reference default 1e-3 without its warm-up scheduler the final ReLU dies after one step on
    synthetic targets -- on the oracle exactly as here, tools/train_trajectory.py.)"""
    from tactilesr_amd import optim
    from tactilesr_amd.train import tactileSR_train as TR
    cfg = dict(patternFeatureExtraLayerCnt=2)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), 42)
    g = torch.Generator().manual_seed(1)
    B, steps, lr = 8, 10, 3e-5
    LR = torch.rand(B, 3, 4, 4, generator=g) * 8
    HR = F.interpolate(LR.mean(1, keepdim=True), size=(100, 100), mode="bilinear") * 30
    p, state, ref = {k: v.clone() for k, v in sd.items()}, {}, []
    for it in range(steps):
        loss, _ = O.train_one_iter(p, state, it + 1, LR, HR, lr=lr, weight_decay=1e-2)
        ref.append(loss)
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    opt = optim.Adam(m.parameters(), lr=lr, weight_decay=1e-2)
    conf = TR.default_config()
    got = [float(TR.train_one_iter(m, opt, (LR, HR), conf)["total_loss"]) for _ in range(steps)]
    rel = [abs(a - b) / abs(a) for a, b in zip(ref, got)]
    print("[trajectory]", ["%.1e" % r for r in rel])
    assert ref[-1] < 0.8 * ref[0]                     # the curve is alive
    assert max(rel[:3]) < 1e-5 and max(rel) < 1e-3, rel


@pytest.mark.filterwarnings("ignore:Detected call of")
def test_trainer_loop_under_warmup_steplr_tracks_the_oracle(T, golden):
    """SURVEY 8(f2) on hardware: three short epochs of the trainer step (train_cal_loss -> zero_grad -> backward -> fused
    Adam-L2) with the learning rate driven by LRWarmupScheduler('auto') in front of StepLR(1, 0.8) exactly as the
    reference's hooks drive it (iter_update after every iteration, epoch_update after every epoch:
    cpu/lr_scheduler.py:97-166, train/tactileSR_train.py:215-228).  The rate the optimizer holds before every iteration
    must be BIT-EQUAL to the sequence the reference's own scheduler class produced (tests/golden/lr_schedule_short.npz:
    warm-up crossing the first epoch end, two StepLR decays), and the loss curve follows the CPU oracle's
    `train_one_iter` fed THAT golden sequence: 1e-5 for the first three steps, then within 3x the oracle's own
    fp32-vs-fp64 drift of this loop (floor 1e-4) -- a bar that the same loop without the two StepLR decays misses by
    more than 10x."""
    from tactilesr_amd import optim
    from tactilesr_amd.train import tactileSR_train as TR
    from tactilesr_amd.train.lr_scheduler import LRWarmupScheduler
    seq = golden("lr_schedule_short")["short_auto"]
    epochs, epoch_len = 3, 6
    assert seq.shape == (1 + epochs * (epoch_len + 1),)
    cfg = dict(patternFeatureExtraLayerCnt=2)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), 42)
    g = torch.Generator().manual_seed(2)
    B = 8
    batches = []
    for _ in range(epoch_len):                                   # a 6-batch "loader", replayed every epoch
        LR = torch.rand(B, 3, 4, 4, generator=g) * 8
        batches.append((LR, F.interpolate(LR.mean(1, keepdim=True), size=(100, 100), mode="bilinear") * 30))
    # oracle: the golden rate of iteration (e, j) is the entry after the previous update, index e*(epoch_len+1)+j
    def oracle_curve(rate, f64=False):
        p = {k: (v.clone().double() if f64 and v.is_floating_point() else v.clone()) for k, v in sd.items()}
        state, curve, step = {}, [], 0
        for e in range(epochs):
            for j, (LR, HR) in enumerate(batches):
                step += 1
                lr = rate(e, j)
                if not f64:
                    curve.append(O.train_one_iter(p, state, step, LR, HR, lr=lr, weight_decay=1e-2)[0])
                    continue
                # the same step in fp64 (O.train_cal_loss casts to fp32 like the reference's .type(torch.float32))
                leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items() if O.is_trainable(k)}
                full = dict(p)
                full.update(leaves)
                ns = {}
                loss = F.mse_loss(O.tactilesr_forward(full, LR.double(), training=True, new_stats=ns),
                                  O.prepare_target(HR).double())
                gl = torch.autograd.grad(loss, list(leaves.values()))
                for k, v in ns.items():
                    p[k] = v.detach()
                O.adam_l2_step(p, dict(zip(leaves, gl)), state, step, lr, 1e-2)
                curve.append(float(loss.detach()))
        return curve, p

    golden_rate = lambda e, j: float(seq[e * (epoch_len + 1) + j])            # noqa: E731
    ref, p = oracle_curve(golden_rate)
    ref64, p64 = oracle_curve(golden_rate, f64=True)
    # control: the same loop WITHOUT the StepLR decays (the rate held at its end-of-warm-up value)
    held, _ = oracle_curve(lambda e, j: float(seq[min(e * (epoch_len + 1) + j, 9)]))
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    opt = optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-2)
    sch = LRWarmupScheduler(torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.8), by_epoch=True,
                            epoch_len=epoch_len, warmup_t=8, warmup_by_epoch=False, warmup_mode="auto",
                            warmup_init_lr=1e-5, warmup_factor=1e-2)
    conf = TR.default_config()
    got, used = [], []
    for e in range(epochs):
        for j, batch in enumerate(batches):
            used.append(opt.param_groups[0]["lr"])
            assert used[-1] == seq[e * (epoch_len + 1) + j], (e, j, used[-1])
            got.append(float(TR.train_one_iter(m, opt, batch, conf)["total_loss"]))
            sch.iter_update()
        sch.epoch_update()
    assert opt.param_groups[0]["lr"] == seq[-1]
    assert len(set(used)) >= 9                                    # the rate really moved: ramp + two decays
    rel = [abs(a - b) / abs(a) for a, b in zip(ref, got)]
    # Yardstick: the training trajectory amplifies rounding (Adam's first steps move every weight by +-lr whatever the
    # gradient's size, ReLU masks flip) -- the oracle's OWN fp32 and fp64 runs of this loop drift apart to 6e-4 by step
    # 18.  Bars: 1e-5 for the first three steps; afterwards no further from the oracle's fp32 curve (and from its fp64
    # curve) than 3x the largest fp32-vs-fp64 distance the oracle itself has shown up to that step (floor 1e-4).
    drift = [abs(a - b) / abs(b) for a, b in zip(ref, ref64)]
    rel64 = [abs(a - b) / abs(a) for a, b in zip(ref64, got)]
    print("[trainer loop under warm-up + StepLR] hip vs oracle fp32 ", ["%.1e" % r for r in rel])
    print("[trainer loop under warm-up + StepLR] hip vs oracle fp64 ", ["%.1e" % r for r in rel64])
    print("[trainer loop under warm-up + StepLR] oracle fp32 vs fp64", ["%.1e" % r for r in drift])
    assert max(rel[:3]) < 1e-5, rel
    for i in range(len(got)):
        bar = max(1e-4, 3 * max(drift[:i + 1]))
        assert rel[i] <= bar and rel64[i] <= bar, (i, rel[i], rel64[i], bar)
    # ... and that bar still SEES the schedule: dropping only the two StepLR decays moves the oracle's final loss by
    # more than ten times the distance between the HIP curve and the oracle's
    miss = abs(held[-1] - ref[-1]) / abs(ref[-1])
    print(f"[trainer loop under warm-up + StepLR] final loss without the StepLR decays: {miss:.1e} away")
    assert ref[-1] < 0.7 * ref[0] and miss > 10 * max(rel[-1], rel64[-1]), (miss, rel[-1])
    # the weights the schedule produced: the post-loop running statistics agree with the oracle's to the same yardstick
    # (the oracle's own fp32-vs-fp64 distance on that tensor after the 18 steps, x3, floor 1e-4)
    new_sd = m.state_dict()
    for k in [k for k in p if k.endswith("running_mean") or k.endswith("running_var")]:
        bar = max(1e-4, 3 * relerr(p[k], p64[k]))
        assert relerr(new_sd[k], p[k]) <= bar, (k, relerr(new_sd[k], p[k]), bar)


def test_seqs_transplant_forward_backward_frozen_blocks(T):
    """a12 on hardware (reference train/tactileSRSeqs_train.py:43-59,74-77): T=7 model, optimizer built BEFORE
    ``model_param_init`` swaps in the single-frame model's feature extractors.  After the swap the engine must run
    the transplanted modules (weight packs follow the new module objects), every live parameter gets an on-pattern
    fp64-grade gradient, the optimizer (which still holds the discarded modules' parameters) leaves the transplanted
    blocks frozen while their BatchNorm running statistics move, and the stems / fuse / head do train."""
    from tactilesr_amd import optim
    from tactilesr_amd.train import checkpoint as CK
    cfg7 = dict(seqsCnt=7, patternFeatureExtraLayerCnt=2)
    cfg1 = dict(seqsCnt=1, patternFeatureExtraLayerCnt=2)
    sd7 = O.random_state_dict(O.tactilesr_state_shapes(**cfg7), 701)
    sd1 = O.random_state_dict(O.tactilesr_state_shapes(**cfg1), 702)
    m = T.TactileSR(**cfg7)
    m.load_state_dict(sd7, strict=True)
    m = m.cuda().train()
    g = torch.Generator().manual_seed(703)
    LR, HR = torch.rand(3, 21, 4, 4, generator=g) * 8, torch.rand(3, 1, 40, 40, generator=g) * 25
    F.mse_loss(m(LR.cuda()), HR.cuda()).backward()             # engine + weight packs exist for the OLD modules
    opt = optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-2)
    old_block_params = [p for p in m.patternFeatureExtra_layer.parameters()]
    CK.model_param_init(m, sd1, lambda: T.TactileSR(**cfg1))
    assert all(p is not q for p, q in zip(m.patternFeatureExtra_layer.parameters(), old_block_params))
    # the state dict the oracle sees = seqs stems/fuse/head + transplanted single-frame blocks
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for k in sd:
        if k.startswith("patternFeatureExtra_layer") or k.startswith("forceFeatureExtra_layer"):
            assert torch.equal(sd[k], sd1[k]), k
    eng = _debug_engine(m)
    opt.zero_grad()
    out = m(LR.cuda())
    loss = F.mse_loss(out, HR.cuda())
    l64, _, ns64, pre64 = GC.oracle_grads(sd, LR, HR, record=True)
    assert abs(loss.item() - l64) < 1e-5 * abs(l64)
    loss.backward()
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    GC.check_pattern(masks, pre64)
    _, g64m, _, _ = GC.oracle_grads(sd, LR, HR, masks=masks)
    GC.check_grads({k: p.grad for k, p in m.named_parameters()}, g64m, tol=1e-5)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt.step()
    after = m.state_dict()
    for k in before:
        moved = not torch.equal(before[k], after[k])
        in_blocks = k.startswith("patternFeatureExtra_layer") or k.startswith("forceFeatureExtra_layer")
        if in_blocks:
            assert not moved, f"{k}: transplanted block must stay frozen (optimizer holds the discarded modules)"
        elif O.is_trainable(k):
            assert moved, f"{k}: live parameter did not train"
    for k, v in ns64.items():                                   # BN statistics of frozen blocks still move
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert relerr(after[k], v) < 1e-5, k
    m.eval()
    with torch.no_grad():
        ref = O.tactilesr_forward({k: v.cpu() for k, v in after.items()}, LR)
    assert relerr(m(LR.cuda()), ref) < 1e-5                     # eval plan re-packed from the transplanted modules


def test_fused_multi_tensor_adam_matches_torch_adam_in_one_launch_per_step():
    """tactilesr_amd.optim.Adam (ONE tsr_adam_l2_multi launch per step over all tensors) against torch.optim.Adam
    (L2-in-gradient weight decay) on CPU: ragged sizes, a 4-byte-misaligned view, a parameter that never gets a
    gradient (skipped like torch skips it), five steps with a changing learning rate."""
    from tactilesr_amd import optim
    g = torch.Generator().manual_seed(9)
    shapes = [(128, 128, 5, 5), (64, 256, 1, 1), (64,), (1, 128, 3, 3), (4097,), (3,), (5000,)]
    cpu = [torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in shapes]
    backing = torch.zeros(5001, device="cuda")
    dev = [torch.nn.Parameter(p.detach().clone().cuda()) for p in cpu[:-1]]
    odd = torch.nn.Parameter(backing[1:])                          # data_ptr % 16 == 4: scalar path
    with torch.no_grad():
        odd.copy_(cpu[-1])
    dev.append(odd)
    frozen_c, frozen_d = torch.nn.Parameter(torch.ones(7)), torch.nn.Parameter(torch.ones(7, device="cuda"))
    # yardstick: torch's Adam in float64 on the same data.  Where g + wd*w cancels to ~eps the step m/(sqrt(v)+eps) is
    # ill-conditioned and torch's own fp32 run is ~1e-5 off its fp64 run; the HIP result must be as close (x4).
    cpu64 = [torch.nn.Parameter(p.detach().double()) for p in cpu]
    ref64 = torch.optim.Adam(cpu64, lr=1e-3, weight_decay=1e-2)
    ref = torch.optim.Adam(cpu + [frozen_c], lr=1e-3, weight_decay=1e-2)
    opt = optim.Adam(dev + [frozen_d], lr=1e-3, weight_decay=1e-2)
    for it in range(5):
        for pg in (ref.param_groups[0], opt.param_groups[0], ref64.param_groups[0]):
            pg["lr"] = 1e-3 * (0.5 + it)
        for pc, pd, p64 in zip(cpu, dev, cpu64):
            gr = torch.randn(pc.shape, generator=g) * (10.0 ** (it - 3))
            pc.grad, pd.grad, p64.grad = gr.clone(), gr.cuda(), gr.double()
        ref.step()
        ref64.step()
        opt.step()
        assert opt.launches == it + 1
        for pc, pd, p64 in zip(cpu, dev, cpu64):
            e_hip, e_ref = relerr(pd, p64), relerr(pc, p64)
            assert e_hip <= max(1e-6, 4 * e_ref), (it, tuple(pc.shape), e_hip, e_ref)
    assert torch.equal(frozen_d.cpu(), frozen_c.detach()) and len(opt.state[frozen_d]) == 0
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 5
    assert relerr(sd["state"][0]["exp_avg_sq"], ref.state_dict()["state"][0]["exp_avg_sq"]) < 1e-6


def test_gradient_arena_and_inbackward_bucket_allreduce_on_the_hip_engine(T):
    """The data-parallel machinery on the real engine, single-rank RCCL group (the pool gives one GPU): weight
    gradients are reduced straight into the arena (p.grad aliases it: no copies), from the second step on every bucket's
    all-reduce is enqueued from INSIDE backward, in production order, and the result equals the un-synced gradient
    (x 1/2: the world size is forced to 2 so that the reduce + mean path really runs; a 1-rank sum is the identity)."""
    import os
    import socket
    import torch.distributed as dist
    from tactilesr_amd import ddp, optim
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    ddp.init_distributed("nccl")
    try:
        cfg = dict(patternFeatureExtraLayerCnt=2)
        sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), 31)
        g = torch.Generator().manual_seed(32)
        LR, HR = (torch.rand(4, 3, 4, 4, generator=g) * 8).cuda(), (torch.rand(4, 1, 40, 40, generator=g) * 25).cuda()

        def fresh():
            m = T.TactileSR(**cfg)
            m.load_state_dict(sd, strict=True)
            return m.cuda().train()

        ref = fresh()
        F.mse_loss(ref(LR), HR).backward()
        ref_g = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
        m = fresh()
        sync = ddp.GradSync(m)
        assert sync.world == 1 and dist.get_backend() == "nccl"
        sync.world = 2
        named = dict(m.named_parameters())
        for step in range(3):
            for p in m.parameters():
                p.grad = None
            with torch.no_grad():                       # same weights and BN statistics every step
                m.load_state_dict(sd, strict=True)
            sync.events.clear()
            F.mse_loss(m(LR), HR).backward()
            ev = list(sync.events)
            arena = m.train_engine().arena
            assert all(named[n].grad.data_ptr() == arena.flat.data_ptr() + 4 * arena.offsets[n] for n in arena.names), \
                "autograd did not adopt the arena views"
            sync.finish()
            nb = len(arena.buckets)
            if step == 0:
                assert ev == [] and [e[0] for e in sync.events[:nb]] == ["enqueue_late"] * nb
            else:
                assert ev == [("enqueue", k) for k in range(nb)], ev
            torch.cuda.synchronize()
            for k, p in named.items():
                assert torch.equal(p.grad, ref_g[k] * 0.5), (step, k)
        assert 2 <= nb <= 8 and set(arena.names) == set(named)      # buckets are cut at tensor boundaries
        # production order: the head's gradients come first, the stems' last
        assert arena.names[0] == "output_layer.2.weight" and arena.names[-1] == "inputLayer_pattern_list.0.1.weight"
        # the fused Adam then steps from the arena with a table that is built once
        opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
        opt.step()
        n_tables = len(opt._tables)
        for p in m.parameters():
            p.grad = None
        F.mse_loss(m(LR), HR).backward()
        sync.finish()
        opt.step()
        assert len(opt._tables) == n_tables == 1 and opt.launches == 2 and opt.table_builds == 1
    finally:
        dist.destroy_process_group()
