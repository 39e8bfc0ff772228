"""GPU parity tests proper (run with -m gpu on an MI355X): every HIP entry point is
called through the C ABI and compared with the CPU oracle / golden fixtures.
Tolerance (north_star): 1e-5 relative fp32, measured as max|y-ref| / max|ref| per tensor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O
import _gradcheck as GC

pytestmark = pytest.mark.gpu
TOL = 1e-5


def relerr(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd
    from tactilesr_amd import _lib
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return M


CONV_CASES = [
    # ks, cin, cout, B, H, W, scale/shift, residual, relu
    (3, 64, 64, 2, 40, 40, True, False, True),
    (5, 64, 64, 3, 40, 40, True, False, True),
    (3, 128, 128, 2, 40, 40, True, False, True),
    (5, 128, 128, 1, 40, 40, True, False, True),
    (1, 256, 64, 3, 40, 40, True, True, True),
    (3, 64, 64, 2, 40, 40, False, True, True),
    (3, 128, 128, 2, 40, 40, False, False, False),
    (3, 448, 64, 1, 40, 40, True, False, True),     # T=7 fuse conv
    (5, 16, 64, 5, 13, 21, True, True, False),      # ragged spatial, odd batch, one block
    (3, 32, 128, 1, 100, 100, True, False, True),   # sf=25 image size (partial tiles)
    (1, 64, 128, 2, 8, 8, False, False, False),
]


@pytest.mark.parametrize("ks,cin,cout,B,H,W,affine,residual,relu", CONV_CASES)
def test_conv2d_fwd(T, ks, cin, cout, B, H, W, affine, residual, relu):
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(ks * 1000 + cin + cout + B)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cout * ks * ks)) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5 if affine else None
    shift = torch.randn(cout, generator=g) * 0.3 if affine else None
    res = torch.randn(B, cout, H, W, generator=g) if residual else None
    ref = F.conv2d(x, w, None, padding=ks // 2)
    if affine:
        ref = ref * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if residual:
        ref = ref + res
    if relu:
        ref = F.relu(ref)
    # write into a channel slice of a wider buffer to exercise ctot/coff (cat elision)
    out_ctot, out_coff = cout + 32, 16
    in_ctot, in_coff = cin + 16, 16
    dev = "cuda"
    xin = T.to_cb16(x.to(dev), in_ctot, in_coff)
    wp = torch.empty_like(w, device=dev)
    wd = w.to(dev).contiguous()
    call("tsr_pack_conv_weight", ptr(wd), ptr(wp), I(cout), I(cin), I(ks), stream())
    out = torch.full((B * out_ctot * H * W,), float("nan"), device=dev)
    rbuf = T.to_cb16(res.to(dev), cout + 16, 16) if residual else None
    sc = scale.to(dev) if affine else None
    sh = shift.to(dev) if affine else None
    call("tsr_conv2d_fwd", ptr(xin), I(in_ctot), I(in_coff), I(cin), ptr(wp), I(cout), I(ks), ptr(sc), ptr(sh),
         ptr(rbuf), I(cout + 16 if residual else 0), I(16 if residual else 0), ptr(out), I(out_ctot), I(out_coff),
         I(int(relu)), I(B), I(H), I(W), stream())
    got = T.from_cb16(out, B, cout, H, W, out_ctot, out_coff)
    assert relerr(got, ref) < TOL
    # channels outside the slice must be untouched
    guard = T.from_cb16(out, B, 16, H, W, out_ctot, 0)
    assert torch.isnan(guard).all()


@pytest.mark.parametrize("sf,B,coff,ctot", [(10, 3, 0, 3), (10, 2, 3, 21), (25, 2, 0, 3)])
def test_stem_fwd(T, sf, B, coff, ctot):
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(sf + B)
    lr = torch.rand(B, ctot, 4, 4, generator=g) * 8
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
    scale = torch.rand(64, generator=g) + 0.5
    shift = torch.randn(64, generator=g) * 0.3
    up = O.bilinear_resize(lr[:, coff:coff + 3], (4 * sf, 4 * sf))
    ref = F.relu(F.conv2d(up, w, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    H = W = 4 * sf
    out = torch.zeros(B * 64 * H * W, device="cuda")
    lr_d, w_d, sc_d, sh_d = lr.cuda(), w.cuda(), scale.cuda(), shift.cuda()   # keep alive across the launch
    call("tsr_stem_fwd", ptr(lr_d), I(ctot), I(coff), I(3), I(4), I(4), I(sf), ptr(w_d),
         ptr(sc_d), ptr(sh_d), ptr(out), I(64), I(0), I(1), I(B), ptr(None), stream())
    assert relerr(T.from_cb16(out, B, 64, H, W), ref) < TOL


@pytest.mark.parametrize("B,H,W", [(2, 40, 40), (1, 100, 100), (3, 9, 17)])
def test_head_fwd(T, B, H, W):
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, 128, H, W, generator=g)
    w = torch.randn(1, 128, 3, 3, generator=g) * 0.05
    ref = F.relu(F.conv2d(x, w, padding=1))
    out = torch.zeros(B, 1, H, W, device="cuda")
    x_d, w_d = T.to_cb16(x.cuda()), w.cuda()
    call("tsr_head_fwd", ptr(x_d), I(128), I(128), ptr(w_d), ptr(out), I(1), I(B), I(H), I(W), stream())
    assert relerr(out, ref) < TOL


@pytest.mark.parametrize("B,C,H,W,relu", [(2, 128, 40, 40, 1), (1, 128, 100, 100, 1), (3, 128, 9, 17, 0), (5, 64, 13, 21, 1),
                                          (2, 128, 3, 2, 0), (1, 128, 40, 1000, 1)])
def test_head_fwd_bf16_storage(T, B, C, H, W, relu):
    """The head on a bf16 CB16 input (tsr_head_fwd_b16: MFMA form -- the stored activation is exact in bf16, the fp32 weight
    enters as three bf16 planes -- or, for very wide images, the LDS-tiled form): fp32-grade against the convolution of the
    bf16-ROUNDED input with the fp32 weight in fp64 (1e-5 of the output's scale; ragged sizes, one- and two-band images,
    a C_in of 64, with and without the ReLU)."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(B + H + C)
    x = torch.randn(B, C, H, W, generator=g).bfloat16().float()
    w = torch.randn(1, C, 3, 3, generator=g) * 0.05
    ref = F.conv2d(x.double(), w.double(), padding=1)
    ref = F.relu(ref) if relu else ref
    out = torch.full((B, 1, H, W), float("nan"), device="cuda")
    x_d, w_d = T.to_cb16(x.cuda(), C + 16, 0).to(torch.bfloat16), w.cuda()
    call("tsr_head_fwd_b16", ptr(x_d), I(C + 16), I(C), ptr(w_d), ptr(out), I(relu), I(B), I(H), I(W), stream())
    assert relerr(out, ref) < TOL


GOLD_CFG = {"t1": dict(), "t7": dict(seqsCnt=7), "sf25t8": dict(scale_factor=25, seqsCnt=8),
            "t1_l2": dict(patternFeatureExtraLayerCnt=2)}


def probe(t):
    cs = max(1, t.shape[1] // 4)
    return t[:, ::cs, ::3, ::3].contiguous()


def _golden_eval(T, golden, tag, impl):
    g = golden("eval")
    cfg = GOLD_CFG[tag]
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), int(g[f"{tag}/seed"]))
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.conv_impl = impl
    LR = torch.from_numpy(g[f"{tag}/LR"]).cuda()
    y, stages = m.forward_with_stages(LR)
    for name, t in stages.items():
        ref = torch.from_numpy(g[f"{tag}/stage/{name}/probe"])
        assert relerr(probe(t), ref) < TOL, name
    yard = float(g[f"{tag}/ref32_vs_f64"])
    if tag == "sf25t8":
        e32 = relerr(y[0, 0, ::2, ::2], torch.from_numpy(g[f"{tag}/out_full0"]))
        e64 = relerr(y[0, 0, ::2, ::2], torch.from_numpy(g[f"{tag}/out64_full0"]))
    else:
        e32 = relerr(y, torch.from_numpy(g[f"{tag}/out"]))
        e64 = relerr(y, torch.from_numpy(g[f"{tag}/out64"]))
    print(f"[parity {impl}] {tag}: hip-vs-ref32 {e32:.2e}  hip-vs-f64 {e64:.2e}  ref32-vs-f64 {yard:.2e}")
    assert torch.equal(y, m(LR))
    return e32, e64


@pytest.mark.parametrize("impl", ["fp16x3", "f32", "bf16x6"])
@pytest.mark.parametrize("tag", ["t1", "t1_l2", "t7"])
def test_model_eval_forward_vs_reference_golden(T, golden, tag, impl):
    """HIP eval forward vs outputs of the reference itself (tests/golden/eval.npz), per-stage and final, for the
    default conv arithmetic (fp16x3), the strict fp32-MFMA path and bf16x6, on the shipped shapes (sf=10; T=1, T=7):
    north_star's 1e-5 flat, against the reference's fp32 CPU output AND against the reference run in fp64."""
    e32, e64 = _golden_eval(T, golden, tag, impl)
    assert e32 < TOL and e64 < TOL


@pytest.mark.parametrize("impl", ["fp16x3", "f32", "bf16x6"])
def test_model_eval_forward_sf25_T8_randomised_fixture_relative_bar(T, golden, impl):
    """The configs[4] parametrisation (scale_factor=25, seqsCnt=8) with RANDOMISED BatchNorm gains (tests/golden/eval.npz
    `sf25t8`): the final 128->1 conv is cancellation-heavy there -- the reference's OWN fp32 CPU run is `ref32_vs_f64`
    = 5.2e-6 of the output max away from its fp64 run, so two faithful fp32 evaluations can differ by more than 1e-5.
    Every stage tensor still meets the flat 1e-5 (checked inside _golden_eval).  The final image is held to bars that
    come from the FIXTURE's conditioning, not from a measurement of this build:
      * strict fp32-MFMA path: within 2 x ref32_vs_f64 of the fp64 run (as close to exact arithmetic as twice the
        reference's own fp32 distance) and, by the triangle inequality, within 3 x of the reference's fp32 run;
      * fp16x3 (default) and bf16x6 (cross-check): no further from either reference run than the strict fp32 path
        measured in the same process, + 1e-6 (fp16x3) / + 5e-6 (bf16x6) -- the split paths can never drift away from
        fp32-MFMA arithmetic unnoticed.
    The well-conditioned configs[4] fixture (the reference's own seed-42 parameters) is held to the flat 1e-5 in
    test_model_eval_forward_reference_init_fixture."""
    g = golden("eval")
    yard = float(g["sf25t8/ref32_vs_f64"])
    e32_f, e64_f = _golden_eval(T, golden, "sf25t8", "f32")
    assert e64_f <= 2 * yard and e32_f <= 3 * yard, (e32_f, e64_f, yard)
    if impl != "f32":
        slack = 1e-6 if impl == "fp16x3" else 5e-6
        e32, e64 = _golden_eval(T, golden, "sf25t8", impl)
        assert e32 <= e32_f + slack and e64 <= e64_f + slack, (impl, e32, e64, e32_f, e64_f)


INIT_CFG = {"init_t1": dict(), "init_sf25t8": dict(scale_factor=25, seqsCnt=8)}


def _init_fixture_model(T, g, tag):
    """The reference's own parameters: seed-42 construction (bit-identical to the reference's, tests/test_host_cpu.py and
    the sha256 below) + the BatchNorm running statistics its two train-mode passes produced (tests/golden/eval_init.npz)."""
    import hashlib
    torch.manual_seed(42)
    m = T.TactileSR(**INIT_CFG[tag])
    h = hashlib.sha256()
    sd = m.state_dict()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().numpy().tobytes())
    assert h.hexdigest() == str(g[f"{tag}/sha256_init"])
    sd = {k: (torch.from_numpy(g[f"{tag}/stat/{k}"]) if f"{tag}/stat/{k}" in g.files else v.clone()) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    return m, sd


@pytest.mark.parametrize("impl", ["fp16x3", "f32", "bf16x6"])
@pytest.mark.parametrize("tag", ["init_t1", "init_sf25t8"])
def test_model_eval_forward_reference_init_fixture(T, golden, tag, impl):
    """configs[4] shape (sf=25, T=8; and the shipped sf=10, T=1) with the REFERENCE'S OWN parameters -- `_init_network`
    under seed 42 (model/tactileSR_model.py:92-98), running statistics moved by two train-mode passes of the reference
    -- flat 1e-5 per stage and on the final image, against the reference's fp32 output and its fp64 run."""
    g = golden("eval_init")
    m, _ = _init_fixture_model(T, g, tag)
    m = m.cuda().eval()
    m.conv_impl = impl
    y, stages = m.forward_with_stages(torch.from_numpy(g[f"{tag}/LR"]).cuda())
    for name, t in stages.items():
        assert relerr(probe(t), torch.from_numpy(g[f"{tag}/stage/{name}/probe"])) < TOL, name
    e32, e64 = relerr(y, torch.from_numpy(g[f"{tag}/out"])), relerr(y, torch.from_numpy(g[f"{tag}/out64"]))
    print(f"[parity {impl}] {tag}: hip-vs-ref32 {e32:.2e}  hip-vs-f64 {e64:.2e}  ref32-vs-f64 {float(g[f'{tag}/ref32_vs_f64']):.2e}")
    assert e32 < TOL and e64 < TOL


@pytest.mark.parametrize("impl", ["fp16x3", "f32", "bf16x6"])
def test_batch4096_distinct_frames_wide_amplitude_per_frame_error(T, golden, impl):
    """B = 4096 with 256 DISTINCT frames whose taxel amplitudes span 2^8 (frame k: rand * 8 * 2^-(k mod 9)), tiled 16x,
    loud and quiet frames side by side in the same workgroups.  The fp16x3 operand scale is a tensor-wide max|x|, so a
    quiet frame shares its scale with a loud one: the error is measured PER FRAME against the CPU oracle (fp32 and
    fp64 runs) on the 256 distinct frames -- the whole-tensor max-norm of the other tests is blind to a quiet frame.
      * quiet classes (amplitude <= 2^-5, 113 frames): 1e-5 relative to the frame's OWN output maximum;
      * every frame: 1e-5 relative to max(own maximum, half the median frame maximum).  The floor is there because the
        absolute error of a faithful fp32 evaluation is uniform over the frames (it is set by the magnitude of the
        128 x 9 terms the last conv sums, not by their sum), while a few LOUD frames end in a final ReLU that cancels
        their output to 2-40 % of the usual magnitude (five to all zeros): relative to such a frame's own maximum the
        ORACLE's fp32 run is itself 4e-5 away from its fp64 run (frame 27).  The unfloored figure is printed;
      * frames whose reference output is all zero: absolute error <= 1e-5 of the batch maximum."""
    g = golden("eval_init")
    m, sd = _init_fixture_model(T, g, "init_t1")
    m = m.cuda().eval()
    m.conv_impl = impl
    gen = torch.Generator().manual_seed(2024)
    base = torch.rand(256, 3, 4, 4, generator=gen) * 8
    cls = torch.arange(256) % 9
    base = base * (2.0 ** -cls.float()).view(-1, 1, 1, 1)
    amp = base.abs().amax(dim=(1, 2, 3))
    assert float(amp.max() / amp.min()) >= 2 ** 8 * 0.5
    LR = base.repeat(16, 1, 1, 1)
    assert LR.shape[0] == 4096
    y = m(LR.cuda()).view(16, 256, 1, 40, 40)
    assert torch.equal(y, y[:1].expand_as(y))
    with torch.no_grad():
        ref = O.tactilesr_forward(sd, base).double()
        ref64 = O.tactilesr_forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, base.double())
    got = y[0].cpu().double()
    fmax = ref64.abs().amax(dim=(1, 2, 3))
    live = fmax > 1e-3 * float(fmax.max())
    a32, a64 = (got - ref).abs().amax(dim=(1, 2, 3)), (got - ref64).abs().amax(dim=(1, 2, 3))
    own = fmax.clamp_min(1e-30)
    floored = torch.maximum(fmax, 0.5 * fmax[live].median())
    quiet = live & (cls >= 5)
    print(f"[wide amplitude {impl}] {int(live.sum())} live frames, {int(quiet.sum())} quiet; per-frame error relative to the own "
          f"maximum: quiet classes {float((a32 / own)[quiet].max()):.2e} (fp32 oracle) / {float((a64 / own)[quiet].max()):.2e} (fp64), "
          f"all live frames {float((a32 / own)[live].max()):.2e} / {float((a64 / own)[live].max()):.2e} (oracle fp32 vs fp64: "
          f"{float(((ref - ref64).abs().amax(dim=(1, 2, 3)) / own)[live].max()):.2e}); with the half-median floor "
          f"{float((a32 / floored).max()):.2e} / {float((a64 / floored).max()):.2e}")
    assert int(quiet.sum()) >= 100
    assert float((a32 / own)[quiet].max()) < TOL and float((a64 / own)[quiet].max()) < TOL
    assert float((a32 / floored).max()) < TOL and float((a64 / floored).max()) < TOL
    assert float(a32[~live].max() if (~live).any() else 0.0) <= TOL * float(fmax.max())


def test_non_finite_taxels_stay_in_their_frame_and_reach_the_loss(T, golden):
    """A NaN taxel and an Inf taxel (reference: NaN / Inf propagate through conv, BN and torch's NaN-propagating ReLU
    to the output of THEIR frame; frames are independent in eval mode, model/tactileSR_model.py:67-84; the trainer
    raises FloatingPointError on the non-finite loss, cpu/trainer.py:280-284).  Here: the poisoned frames' outputs are
    non-finite, every other frame of the batch -- including the ones sharing a workgroup with a poisoned frame -- still
    meets 1e-5 against the oracle, and the MSE loss over the batch is non-finite.  (The kernels' ReLU is a select, not
    v_max_f32; padding is a select, not a multiply by 0; non-finite maxima are kept out of the operand scales.)"""
    from tactilesr_amd import functional as Fh
    g = golden("eval_init")
    m, sd = _init_fixture_model(T, g, "init_t1")
    m = m.cuda().eval()
    gen = torch.Generator().manual_seed(77)
    LR = torch.rand(9, 3, 4, 4, generator=gen) * 8
    with torch.no_grad():
        ref_clean = O.tactilesr_forward(sd, LR)
    bad = LR.clone()
    bad[2, 1, 0, 0] = float("nan")          # frame 2 shares its workgroups with frame 3, frame 5 with frame 4
    bad[5, 0, 3, 2] = float("inf")
    bad[6, 2, 1, 1] = float("-inf")
    for impl in ("fp16x3", "f32", "bf16"):
        m.conv_impl = impl
        y = m(bad.cuda()).cpu()
        for b in (2, 5, 6):
            assert not torch.isfinite(y[b]).all(), (impl, b)
        ok = [0, 1, 3, 4, 7, 8]
        assert torch.isfinite(y[ok]).all(), impl
        assert relerr(y[ok], ref_clean[ok]) < (TOL if impl != "bf16" else 5e-2), impl
        loss = Fh.mse_loss(y.cuda(), torch.zeros_like(y).cuda())
        assert not torch.isfinite(loss), impl
    # torch's own answer on the poisoned batch (what the reference computes): same frames non-finite
    with torch.no_grad():
        ref_bad = O.tactilesr_forward(sd, bad)
    assert [bool(torch.isfinite(ref_bad[b]).all()) for b in range(9)] == [b not in (2, 5, 6) for b in range(9)]


def test_model_eval_forward_vs_oracle_odd_batch(T):
    """Fresh seeded input, odd batch (image-pair tail), seeded reference init + trained-like BN stats."""
    torch.manual_seed(42)
    m = T.TactileSR()
    sd = m.state_dict()
    g = torch.Generator().manual_seed(7)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
        elif k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) * 0.5 + 0.75
    m.load_state_dict(sd)
    LR = torch.rand(5, 3, 4, 4, generator=g) * 8
    with torch.no_grad():
        ref = O.tactilesr_forward({k: v.clone() for k, v in sd.items()}, LR)
    y = m.cuda().eval()(LR.cuda())
    assert relerr(y, ref) < TOL
    # weights changed in place -> plan must be rebuilt
    with torch.no_grad():
        m.output_layer[2].weight.mul_(2.0)
    y3 = m(LR.cuda())
    assert relerr(y3, ref * 2) < TOL


def test_model_chunked_batch_and_linearity_property(T):
    """Size-independent properties at a larger batch: chunked passes equal a single pass,
    permuting the batch permutes the output (samples are independent in eval mode)."""
    torch.manual_seed(1)
    m = T.TactileSR(patternFeatureExtraLayerCnt=1).cuda().eval()
    LR = torch.rand(67, 3, 4, 4, device="cuda") * 8
    y = m(LR)
    m.max_images_per_pass = 16
    y2 = m(LR)
    assert torch.equal(y, y2)
    perm = torch.randperm(67, device="cuda")
    y3 = m(LR[perm])
    assert relerr(y3, y[perm]) < 1e-6


BF16S_CASES = [(3, 64, 64, 3, 40, 40), (5, 128, 128, 1, 40, 40), (1, 256, 64, 2, 40, 40), (3, 128, 128, 2, 13, 21),
               (5, 64, 64, 5, 9, 40), (3, 448, 64, 1, 40, 40)]


@pytest.mark.parametrize("nsplit,tol", [(3, 1e-5), (2, 1e-4), (1, 2e-2)])
@pytest.mark.parametrize("ks,cin,cout,B,H,W", BF16S_CASES)
def test_conv2d_fwd_bf16_split(T, ks, cin, cout, B, H, W, nsplit, tol):
    """Split-bf16 MFMA conv: nsplit=3 (six products) must meet the fp32 bar; 2 / 1 are the documented
    reduced-precision modes (tolerance vs the fp32 reference stated here)."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(ks * 100 + cin + B)
    x = torch.randn(B, cin, H, W, generator=g) * 3
    x[0, 0, 0, 0] = 1e4          # wide dynamic range inside one tile
    x[0, 1, 1, 1] = 1e-6
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cout * ks * ks)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    res = torch.randn(B, cout, H, W, generator=g)
    ref64 = F.relu(F.conv2d(x.double(), w.double(), padding=ks // 2) * scale.double().view(1, -1, 1, 1)
                   + shift.double().view(1, -1, 1, 1) + res.double())
    xin, rbuf = T.to_cb16(x.cuda()), T.to_cb16(res.cuda())
    wd = w.cuda().contiguous()
    from tactilesr_amd._lib import load
    wp = torch.empty(load().tsr_conv_weight_bf16s_elems(cout, cin, ks, nsplit), dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_conv_weight_bf16s", ptr(wd), ptr(wp), I(cout), I(cin), I(ks), I(nsplit), stream())
    out = torch.empty(B * cout * H * W, device="cuda")
    sc, sh = scale.cuda(), shift.cuda()
    call("tsr_conv2d_fwd_bf16s", ptr(xin), I(cin), I(0), I(cin), ptr(wp), I(cout), I(ks), I(nsplit), ptr(sc), ptr(sh),
         ptr(rbuf), I(cout), I(0), ptr(out), I(cout), I(0), I(1), I(B), I(H), I(W), stream())
    got = T.from_cb16(out, B, cout, H, W)
    err = relerr(got, ref64)
    if nsplit == 3:
        ref32 = F.relu(F.conv2d(x, w, padding=ks // 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res)
        print(f"[bf16x6] k{ks} {cin}->{cout}: err vs f64 {err:.2e}  (torch fp32 CPU vs f64 {relerr(ref32, ref64):.2e})")
    assert err < tol


@pytest.mark.parametrize("impl", ["bf16x6", "fp16x3"])
@pytest.mark.parametrize("tag", ["t1", "t7", "t1_l2"])
def test_split_operand_paths_agree_with_fp32_mfma_path(T, golden, tag, impl):
    """Two fp32-grade evaluations of the same network (split-operand vs strict fp32 MFMA) agree within the sum of
    their 1e-5 bars."""
    g = golden("eval")
    cfg = GOLD_CFG[tag]
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), int(g[f"{tag}/seed"]))
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.conv_impl = impl
    LR = torch.from_numpy(g[f"{tag}/LR"]).cuda()
    y = m(LR)
    m.conv_impl = "f32"
    assert relerr(y, m(LR)) < 2 * TOL


@pytest.mark.parametrize("impl", ["bf16x6", "f32", "fp16x3"])
def test_full_size_batch4096_tiling_invariance(T, impl):
    """BASELINE configs[1] size (B=4096): the batch is 32 distinct frames tiled 128x.  Samples are independent in
    eval mode, so every replica must be bit-identical to the first, and the 32 distinct outputs must match the
    CPU oracle (which finishes 32 frames in well under a second)."""
    torch.manual_seed(42)
    m = T.TactileSR()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    m.conv_impl = impl
    g = torch.Generator().manual_seed(11)
    base = torch.rand(32, 3, 4, 4, generator=g) * 8
    LR = base.repeat(128, 1, 1, 1).cuda()
    assert LR.shape[0] == 4096
    y = m(LR)
    y = y.view(128, 32, 1, 40, 40)
    assert torch.equal(y, y[:1].expand_as(y))
    with torch.no_grad():
        ref = O.tactilesr_forward(sd, base)
    assert relerr(y[0], ref) < TOL


# + shapes aimed at the K = 32 kernel (C_out = 128, channel blocks in pairs): one block pair, odd batches, partial tiles,
# the sf = 25 image size; and an odd block count (falls back to the 32x32x16 kernel and its pack order)
K32_CASES = [(5, 32, 128, 3, 100, 100), (3, 32, 128, 3, 9, 17), (5, 64, 128, 2, 40, 40), (3, 64, 128, 5, 24, 8),
             (5, 256, 128, 1, 16, 16), (3, 48, 128, 2, 16, 16), (5, 48, 128, 1, 8, 24)]


@pytest.mark.parametrize("ks,cin,cout,B,H,W", BF16S_CASES + K32_CASES)
@pytest.mark.parametrize("outlier", [False, True])
def test_conv2d_fwd_fp16_split(T, ks, cin, cout, B, H, W, outlier):
    """fp16 two-plane split conv (3 products) with power-of-two operand scaling: fp32-grade single-layer accuracy,
    also with a 1e4 outlier and 1e-6 values in the same tensor (dynamic range handling), and the out_amax scalar it
    publishes for its consumer."""
    import math
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_float as Fl
    g = torch.Generator().manual_seed(ks * 100 + cin + B + 5)
    x = torch.randn(B, cin, H, W, generator=g) * 3
    if outlier:
        x[0, 0, 0, 0] = 1e4
        x[0, 1, 1, 1] = 1e-6
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cout * ks * ks)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    res = torch.randn(B, cout, H, W, generator=g)
    ref64 = F.relu(F.conv2d(x.double(), w.double(), padding=ks // 2) * scale.double().view(1, -1, 1, 1)
                   + shift.double().view(1, -1, 1, 1) + res.double())
    ref32 = F.relu(F.conv2d(x, w, padding=ks // 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res)
    xin, rbuf = T.to_cb16(x.cuda()), T.to_cb16(res.cuda())
    wd = w.cuda().contiguous()
    wscale = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    wp = torch.empty(load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 2), dtype=torch.float16, device="cuda")
    call("tsr_pack_conv_weight_f16s", ptr(wd), ptr(wp), I(cout), I(cin), I(ks), Fl(wscale), stream())
    amax_in = x.abs().max().reshape(1).cuda()
    amax_out = torch.zeros(1, device="cuda")
    out = torch.empty(B * cout * H * W, device="cuda")
    sc, sh = scale.cuda(), shift.cuda()
    call("tsr_conv2d_fwd_f16s", ptr(xin), I(cin), I(0), I(cin), ptr(wp), I(cout), I(ks), Fl(1.0 / wscale), ptr(amax_in),
         ptr(amax_out), ptr(sc), ptr(sh), ptr(rbuf), I(cout), I(0), ptr(out), I(cout), I(0), I(1), I(B), I(H), I(W),
         stream())
    got = T.from_cb16(out, B, cout, H, W)
    err = relerr(got, ref64)
    print(f"[fp16x3] k{ks} {cin}->{cout} outlier={outlier}: err vs f64 {err:.2e}  (torch fp32 CPU vs f64 {relerr(ref32, ref64):.2e})")
    assert err < TOL
    assert abs(float(amax_out) - float(got.abs().max())) == 0.0


@pytest.mark.parametrize("ks,cin,cout", [(5, 64, 128), (3, 64, 64), (5, 48, 128), (3, 16, 64)])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_conv2d_fp16_split_non_finite_input_stays_in_its_receptive_field(T, ks, cin, cout, bad):
    """torch's conv propagates a NaN / Inf input element to exactly the outputs whose window covers it.  The split-operand
    kernels read dummy elements for padding and (odd block counts) a phantom channel block against zero weights: neither
    may carry the bad value anywhere else -- every other output must be BIT-identical to the clean run (the operand scale
    comes from the producer's amax scalar, which skips non-finite values: here the clean tensor's)."""
    import math
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_float as Fl
    B, H, W, P = 3, 16, 24, ks // 2
    g = torch.Generator().manual_seed(ks + cin + cout)
    x = torch.randn(B, cin, H, W, generator=g)
    w = (torch.randn(cout, cin, ks, ks, generator=g) * 0.05).cuda().contiguous()
    wscale = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    wp = torch.empty(load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 2), dtype=torch.float16, device="cuda")
    call("tsr_pack_conv_weight_f16s", ptr(w), ptr(wp), I(cout), I(cin), I(ks), Fl(wscale), stream())
    amax_in = x.abs().max().reshape(1).cuda()

    def run(xx):
        out = torch.empty(B * cout * H * W, device="cuda")
        call("tsr_conv2d_fwd_f16s", ptr(T.to_cb16(xx.cuda())), I(cin), I(0), I(cin), ptr(wp), I(cout), I(ks), Fl(1.0 / wscale),
             ptr(amax_in), ptr(None), ptr(None), ptr(None), ptr(None), I(0), I(0), ptr(out), I(cout), I(0), I(0), I(B), I(H),
             I(W), stream())
        return T.from_cb16(out, B, cout, H, W).cpu()

    clean = run(x)
    # pixel (0, 0) of image 1 is also the dummy element its padding slots read; (7, 9) sits inside a tile
    for (b, c, y, xx_) in [(1, 0, 0, 0), (2, cin - 1, 7, 9)]:
        xb = x.clone()
        xb[b, c, y, xx_] = bad
        got = run(xb)
        win = torch.zeros(B, 1, H, W, dtype=torch.bool)
        win[b, 0, max(0, y - P):y + P + 1, max(0, xx_ - P):xx_ + P + 1] = True
        win = win.expand(B, cout, H, W)
        assert not torch.isfinite(got[win]).any(), "every output whose window covers the bad element is non-finite"
        assert torch.equal(got[~win], clean[~win]), "no other output changes"


def test_stem_publishes_amax(T):
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    g = torch.Generator().manual_seed(3)
    lr = (torch.rand(3, 3, 4, 4, generator=g) * 8).cuda()
    w = (torch.randn(64, 3, 3, 3, generator=g) * 0.2).cuda()
    out = torch.zeros(3 * 64 * 1600, device="cuda")
    amax = torch.zeros(1, device="cuda")
    call("tsr_stem_fwd", ptr(lr), I(3), I(0), I(3), I(4), I(4), I(10), ptr(w), ptr(None), ptr(None), ptr(out), I(64),
         I(0), I(1), I(3), ptr(amax), stream())
    assert float(amax) == float(out.max()) > 0


# ---------------------------------------------------------------------------------------------------------------
# bf16 ACTIVATION STORAGE (BASELINE's "bf16" configurations; reduced precision, never the parity path)
# ---------------------------------------------------------------------------------------------------------------
def _to_cb16_bf16(x, ctot=None, coff=0):
    B, C, H, W = x.shape
    ctot = ctot or C
    full = torch.zeros(B, ctot, H * W, device=x.device)
    full[:, coff:coff + C] = x.reshape(B, C, H * W)
    return full.view(B, ctot // 16, 16, H * W).permute(0, 1, 3, 2).contiguous().to(torch.bfloat16).reshape(-1)


def _from_cb16_bf16(t, B, C, H, W, ctot=None, coff=0):
    ctot = ctot or C
    v = t.view(B, ctot // 16, H * W, 16)[:, coff // 16:(coff + C) // 16]
    return v.permute(0, 1, 3, 2).reshape(B, C, H, W).float()


@pytest.mark.parametrize("ks,cin,cout,B,H,W", BF16S_CASES + [(3, 128, 64, 3, 100, 100)])
def test_conv2d_fwd_bf16_storage(T, ks, cin, cout, B, H, W):
    """tsr_conv2d_fwd_b16: bf16 tensors in HBM (input, residual, output), plain bf16 MFMA operands, fp32 accumulate.
    Against fp64 on the bf16-ROUNDED inputs the only errors are the bf16 weights and the output rounding (bar 1e-2);
    channel slices (ctot / coff) and ragged tiles included."""
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I
    g = torch.Generator().manual_seed(ks * 100 + cin + B + 9)
    x = (torch.randn(B, cin, H, W, generator=g) * 3).to(torch.bfloat16).float()
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cout * ks * ks)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    res = torch.randn(B, cout, H, W, generator=g).to(torch.bfloat16).float()
    ref64 = F.relu(F.conv2d(x.double(), w.double(), padding=ks // 2) * scale.double().view(1, -1, 1, 1)
                   + shift.double().view(1, -1, 1, 1) + res.double())
    xin, rbuf = _to_cb16_bf16(x.cuda(), cin + 16, 16), _to_cb16_bf16(res.cuda(), cout + 16, 0)
    wd = w.cuda().contiguous()
    wp = torch.empty(load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 1), dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_conv_weight_bf16s", ptr(wd), ptr(wp), I(cout), I(cin), I(ks), I(1), stream())
    out = torch.full((B * (cout + 32) * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
    sc, sh = scale.cuda(), shift.cuda()
    call("tsr_conv2d_fwd_b16", ptr(xin), I(cin + 16), I(16), I(cin), ptr(wp), I(cout), I(ks), ptr(sc), ptr(sh),
         ptr(rbuf), I(cout + 16), I(0), ptr(out), I(cout + 32), I(16), I(1), I(B), I(H), I(W), stream())
    got = _from_cb16_bf16(out, B, cout, H, W, cout + 32, 16)
    assert relerr(got, ref64) < 1e-2
    assert torch.isnan(_from_cb16_bf16(out, B, 16, H, W, cout + 32, 0)).all()      # outside the slice: untouched


B16K_CASES = [(3, 64, 64, 5, 40, 40), (5, 64, 64, 3, 40, 40), (3, 128, 128, 6, 40, 40), (5, 128, 128, 5, 40, 40),
              (3, 448, 64, 2, 40, 40), (3, 32, 64, 1, 13, 21), (5, 96, 128, 3, 17, 9), (3, 128, 128, 1, 100, 100),
              (5, 64, 128, 9, 3, 5), (3, 160, 128, 7, 8, 8), (5, 512, 128, 1, 9, 33)]      # images smaller than a tile / than the kernel, 16 blocks


@pytest.mark.parametrize("ks,cin,cout,B,H,W", B16K_CASES)
@pytest.mark.parametrize("residual", [True, False])
def test_conv2d_fwd_b16k(T, ks, cin, cout, B, H, W, residual):
    """tsr_conv2d_fwd_b16k (csrc/conv_b16k.hip: 16x16x32 MFMA, channels as rows, LDS-DMA circular halo): bf16 tensors in HBM,
    bf16 operands, fp32 accumulate.  Yardstick: fp64 convolution of the bf16-ROUNDED input and weights, rounded to bf16 once:
    >= 99 % of the outputs identical, the rest within one bf16 ulp (or the fp32-accumulation floor next to the ReLU's zero).
    Channel slices (ctot / coff), ragged tiles, batch tails, 1..14 channel blocks; nothing outside the slice is written."""
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I
    g = torch.Generator().manual_seed(ks * 100 + cin + B + 11)
    x = (torch.randn(B, cin, H, W, generator=g) * 3).to(torch.bfloat16).float()
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    res = torch.randn(B, cout, H, W, generator=g).to(torch.bfloat16).float()
    ref = F.conv2d(x.double(), w.bfloat16().double(), padding=ks // 2) * scale.double().view(1, -1, 1, 1) \
        + shift.double().view(1, -1, 1, 1)
    if residual:
        ref = ref + res.double()
    ref = F.relu(ref).float().bfloat16().float()
    xin, rbuf = _to_cb16_bf16(x.cuda(), cin + 16, 16), _to_cb16_bf16(res.cuda(), cout + 16, 0)
    wd = w.cuda().contiguous()
    wp = torch.empty(load().tsr_conv_weight_b16k_elems(cout, cin, ks), dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_conv_weight_b16k", ptr(wd), ptr(wp), I(cout), I(cin), I(ks), stream())
    out = torch.full((B * (cout + 32) * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
    sc, sh = scale.cuda(), shift.cuda()
    call("tsr_conv2d_fwd_b16k", ptr(xin), I(cin + 16), I(16), I(cin), ptr(wp), I(cout), I(ks), ptr(sc), ptr(sh),
         ptr(rbuf if residual else None), I(cout + 16), I(0), ptr(out), I(cout + 32), I(16), I(1), I(B), I(H), I(W), stream())
    got = _from_cb16_bf16(out, B, cout, H, W, cout + 32, 16).cpu()
    ulp = (ref.abs() * 2.0 ** -7).clamp_min(1e-30)
    d = (got - ref).abs()
    same = float((d == 0).float().mean())
    floor = 3e-6 * float(ref.abs().max())
    bad = d > torch.maximum(1.01 * ulp, torch.full_like(ulp, floor))
    print(f"[b16k] k{ks} {cin}->{cout} B={B} {H}x{W} res={residual}: identical {same:.5f}, beyond one ulp: {int(bad.sum())}")
    assert same >= 0.99 and not bad.any()
    assert torch.isnan(_from_cb16_bf16(out, B, 16, H, W, cout + 32, 0)).all()      # outside the slice: untouched
    assert torch.isnan(_from_cb16_bf16(out, B, 16, H, W, cout + 32, cout + 16)).all()


@pytest.mark.parametrize("ks,B,H,W,relu2,with_res,with_bias", [(3, 5, 40, 40, False, True, True), (5, 6, 40, 40, True, True, False),
                                                               (3, 2, 13, 21, True, False, True), (5, 1, 100, 100, True, True, True)])
def test_conv2d_fwd_b16k_fuse1x1(T, ks, B, H, W, relu2, with_res, with_bias):
    """tsr_conv2d_fwd_b16k_fuse1x1: stage-2 conv (128 -> 128, folded BN, ReLU) whose bf16-rounded result feeds, as it sits in the
    accumulator registers, the 64x128 half of the MSRB's 1x1 `confusion` (+ bias + residual, optional ReLU).  Yardstick: the
    same two steps in fp64 on the bf16-rounded operands with the intermediate rounded to bf16 once.  A rounding-boundary
    flip of an intermediate element (fp32 vs fp64 accumulation) moves an output by a fraction of its ulp: >= 98 % identical,
    everything within two ulps or 2e-3 of the tensor maximum."""
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I
    cin = 128
    g = torch.Generator().manual_seed(ks * 10 + B + H)
    x = (torch.randn(B, cin, H, W, generator=g).clamp_(min=0) * 2).bfloat16()
    w = torch.randn(128, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    w2 = torch.randn(64, 128, generator=g) * (1.0 / 128) ** 0.5
    scale, shift = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.3
    shift2 = torch.randn(64, generator=g) * 0.2
    res = torch.randn(B, 64, H, W, generator=g).bfloat16()
    t = F.relu(F.conv2d(x.double(), w.bfloat16().double(), padding=ks // 2) * scale.double().view(1, -1, 1, 1)
               + shift.double().view(1, -1, 1, 1)).float().bfloat16().double()
    ref = torch.einsum("oc,bchw->bohw", w2.bfloat16().double(), t)
    if with_bias:
        ref = ref + shift2.double().view(1, -1, 1, 1)
    if with_res:
        ref = ref + res.double()
    if relu2:
        ref = F.relu(ref)
    ref = ref.float().bfloat16().float()
    xin = _to_cb16_bf16(x.float().cuda())
    rbuf = _to_cb16_bf16(res.float().cuda(), 80, 16)
    wp = torch.empty(load().tsr_conv_weight_b16k_elems(128, cin, ks), dtype=torch.bfloat16, device="cuda")
    wd, w2d = w.cuda().contiguous(), w2.cuda().contiguous()
    call("tsr_pack_conv_weight_b16k", ptr(wd), ptr(wp), I(128), I(cin), I(ks), stream())
    w2p = torch.empty(64 * 128, dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_w2_b16k", ptr(w2d), ptr(w2p), stream())
    out = torch.full((B * 96 * H * W,), float("nan"), dtype=torch.bfloat16, device="cuda")
    sc, sh, sh2 = scale.cuda(), shift.cuda(), shift2.cuda()
    call("tsr_conv2d_fwd_b16k_fuse1x1", ptr(xin), I(cin), I(0), I(cin), ptr(wp), I(ks), ptr(sc), ptr(sh), I(1), ptr(w2p),
         ptr(sh2 if with_bias else None), ptr(rbuf if with_res else None), I(80), I(16), ptr(out), I(96), I(16),
         I(1 if relu2 else 0), I(B), I(H), I(W), stream())
    got = _from_cb16_bf16(out, B, 64, H, W, 96, 16).cpu()
    ulp = (ref.abs() * 2.0 ** -7).clamp_min(1e-30)
    d = (got - ref).abs()
    same = float((d == 0).float().mean())
    mx = float(ref.abs().max())
    bad = d > torch.maximum(2.01 * ulp, torch.full_like(ulp, 2e-3 * mx))
    print(f"[b16k fused] k{ks} B={B} {H}x{W}: identical {same:.5f}, worst {float(d.max()) / mx:.2e} of max, beyond bar: {int(bad.sum())}")
    assert same >= 0.98 and not bad.any()
    assert torch.isnan(_from_cb16_bf16(out, B, 16, H, W, 96, 0)).all() and torch.isnan(_from_cb16_bf16(out, B, 16, H, W, 96, 80)).all()


@pytest.mark.parametrize("tag", ["t1", "t7", "t1_l2", "sf25t8"])
def test_model_eval_forward_bf16_storage_vs_reference_golden(T, golden, tag):
    """conv_impl = 'bf16': every activation between the kernels is a bf16 tensor.  Stated tolerance of BASELINE's bf16
    configurations (the reference has no bf16 numerics to match), against the reference's own fp32 output: 3e-2 of the
    tensor max per stage, 5e-2 on the final image of these randomised-parameter fixtures (their last conv is
    cancellation-heavy).  The per-stage figure is an extreme-value statistic of ~30 layers of accumulated 8-bit roundings:
    three builds of this path whose fp32 summation ORDER differs (all >= 99.5 % element-identical to the emulating oracle
    stage by stage, see the next test) gave 2.4e-2, 2.9e-2 and 3.3e-2 at `head0` of fixture t1.  So the yardstick of a
    stage is the EMULATING ORACLE's own distance from the reference's fp32 value at that stage (exact products, wide
    accumulation: the bf16 arithmetic itself, no kernel in it): a stage may be no further than 3e-2 or 1.5x that distance,
    whichever is larger (measured: worst stage 1.6-3.3e-2 against 1.7-3.7e-2 for the oracle; final 2.0-4.3e-2; seeded
    reference init at B = 4096: 2.2e-2)."""
    g = golden("eval")
    cfg = GOLD_CFG[tag]
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), int(g[f"{tag}/seed"]))
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.conv_impl = "bf16"
    LR = torch.from_numpy(g[f"{tag}/LR"]).cuda()
    y, stages = m.forward_with_stages(LR)
    emu = {}
    with torch.no_grad():
        y_emu = O.tactilesr_forward(sd, LR.cpu(), cfg.get("scale_factor", 10), stages=emu, emulate="bf16")
    worst = worst_emu = 0.0
    for name, t in stages.items():
        ref = torch.from_numpy(g[f"{tag}/stage/{name}/probe"])
        e, e_emu = relerr(probe(t), ref), relerr(probe(emu[name]), ref)
        worst, worst_emu = max(worst, e), max(worst_emu, e_emu)
        assert e < max(3e-2, 1.5 * e_emu), (name, e, e_emu)
    # (the sf = 25 fixture holds every second pixel of the first image)
    def final_err(t):
        return relerr(t[0, 0, ::2, ::2], torch.from_numpy(g[f"{tag}/out_full0"])) if tag == "sf25t8" else relerr(t, torch.from_numpy(g[f"{tag}/out"]))
    e, e_emu = final_err(y), final_err(y_emu)
    print(f"[bf16 storage] {tag}: final {e:.2e} (emulating oracle {e_emu:.2e}), worst stage {worst:.2e} (emulating oracle vs fp32: "
          f"worst stage {worst_emu:.2e})")
    # measured 2.0-5.3e-2 (the oracle: 2.1-5.1e-2): ~30 layers of 8-bit significands in front of a cancellation-heavy head; the
    # same yardstick as for the stages
    assert e < max(5e-2, 1.5 * e_emu)
    assert torch.equal(y, m(LR))


@pytest.mark.parametrize("tag", ["t1", "t7", "t1_l2", "sf25t8"])
def test_model_eval_forward_bf16_storage_vs_bf16_emulating_oracle(T, golden, tag):
    """conv_impl = 'bf16' against the oracle's restatement of ITS arithmetic (`emulate="bf16"`: bf16 rounding of every
    stored activation and of the conv weights, exact products, wide accumulation, fp32 epilogues) -- the reference has
    no bf16 numerics, so this is the check that no tap, halo column or channel is dropped in the bf16 kernels, which a
    3e-2 bar against fp32 cannot see.

    (1) TEACHER-FORCED, per stage: the oracle evaluates every stage on the DEVICE's input of that stage.  Device and
        oracle then differ only where an fp32 pre-rounding value sits within accumulation-order noise (~1e-6 relative)
        of a bf16 rounding boundary and the two round to neighbouring bf16 values (probability ~2e-4 per element and
        rounding), plus -- inside an MSRB, which rounds four times (cat1, the two stage-2 tiles, the partial sum) before
        its output is stored -- the few-layer cascade of such flips through the 1x1 (|w| ~ 0.2):
          * >= 99 % of the elements are IDENTICAL (a dropped tap or halo column changes essentially all of them);
          * >= 99.9 % lie within one bf16 ulp of the oracle's value (+ 2e-4 of the stage maximum);
          * every element lies within 1e-2 of the stage maximum and the relative L2 error is <= 1e-3.
    (2) END TO END, informational: two bf16 evaluations whose roundings differ at a few elements decorrelate layer by
        layer (a pre-rounding difference d flips a rounding with probability d / ulp) until they differ like independent
        roundings do, and the differences then add up over the ~30 layers like the rounding noise itself: measured
        relative L2 2.7e-3 after the second MSRB, 4.7e-3 after the third.  So an end-to-end comparison with the emulating
        oracle says no more than the comparison with fp32 does; it is held to the same stated 3e-2 and printed.  (1) is
        the parity check.
    The old 3e-2-vs-fp32 figure is printed for information."""
    g = golden("eval")
    cfg = GOLD_CFG[tag]
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), int(g[f"{tag}/seed"]))
    LRc = torch.from_numpy(g[f"{tag}/LR"])
    # (the sf = 25 fixture's randomised BatchNorm gains make its 128 -> 1 head cancellation-heavy -- the reference's own fp32
    #  run is 5e-6 from its fp64 run there, ten times the usual: its final image is printed, its stages are held to the bar)
    w_same, w_ulp, w_max, w_l2, e2e_l2, e2e_max, y = GC.bf16_eval_vs_emulating_oracle(T, cfg, sd, LRc,
                                                                                      exempt_e2e_out=tag == "sf25t8")
    print(f"[bf16 vs bf16-oracle] {tag}: teacher-forced worst share of differing elements {w_same:.2e}, beyond one ulp "
          f"{w_ulp:.2e}, worst max-norm {w_max:.2e}, worst rel-L2 {w_l2:.2e}; end-to-end worst rel-L2 {e2e_l2:.2e}, worst "
          f"max-norm {e2e_max:.2e}; vs the reference's fp32 output (information) "
          f"{(relerr(y[0, 0, ::2, ::2], torch.from_numpy(g[f'{tag}/out_full0'])) if tag == 'sf25t8' else relerr(y, torch.from_numpy(g[f'{tag}/out']))):.2e}")


def test_bf16_storage_batch4096_tiling_invariance(T):
    """BASELINE configs[2]-style size for the bf16 path (B = 4096 = 32 frames x 128): replicas bit-identical, the 32
    distinct outputs within 3e-2 of the CPU oracle."""
    torch.manual_seed(42)
    m = T.TactileSR()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    m.conv_impl = "bf16"
    g = torch.Generator().manual_seed(11)
    base = torch.rand(32, 3, 4, 4, generator=g) * 8
    y = m(base.repeat(128, 1, 1, 1).cuda()).view(128, 32, 1, 40, 40)
    assert torch.equal(y, y[:1].expand_as(y))
    with torch.no_grad():
        ref = O.tactilesr_forward(sd, base)
    e = relerr(y[0], ref)
    print(f"[bf16 storage] B=4096: {e:.2e}")
    assert e < 3e-2


@pytest.mark.parametrize("ks,cin,B,H,W,relu2,with_res,with_bias", [
    (3, 128, 2, 40, 40, False, True, True), (5, 128, 3, 40, 40, True, True, False), (5, 128, 1, 13, 21, True, False, True),
    (3, 128, 5, 100, 100, True, True, True), (3, 48, 2, 16, 24, False, False, False)])
def test_conv2d_fused_1x1_epilogue(T, ks, cin, B, H, W, relu2, with_res, with_bias):
    """tsr_conv2d_fwd_f16s_fuse1x1: stage-2 conv (-> 128 ch, BN fold + ReLU) with a 64x128 1x1 GEMM, bias, residual and
    optional ReLU applied before the tile leaves the workgroup -- against fp64, fp32-grade bar, ragged tiles and odd
    batches (out-of-image pixels of a partial tile must not leak into the tile-local operand scale or the output)."""
    import math
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_float as Fl
    g = torch.Generator().manual_seed(ks * 31 + cin + B + H)
    x = torch.randn(B, cin, H, W, generator=g) * 2
    w = torch.randn(128, cin, ks, ks, generator=g) * (2.0 / (128 * ks * ks)) ** 0.5
    scale, shift = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.3
    w2 = torch.randn(64, 128, 1, 1, generator=g) * (2.0 / 64) ** 0.5
    b2 = torch.randn(64, generator=g) * 0.2 if with_bias else None
    res = torch.randn(B, 64, H, W, generator=g) if with_res else None
    a = F.relu(F.conv2d(x.double(), w.double(), padding=ks // 2) * scale.double().view(1, -1, 1, 1)
               + shift.double().view(1, -1, 1, 1))
    ref = F.conv2d(a, w2.double(), b2.double() if with_bias else None)
    if with_res:
        ref = ref + res.double()
    if relu2:
        ref = F.relu(ref)
    lib = load()

    def pack(wt, cout, cin_, k):
        ws = 2.0 ** (13 - math.floor(math.log2(float(wt.abs().max()))))
        wp = torch.empty(lib.tsr_conv_weight_bf16s_elems(cout, cin_, k, 2), dtype=torch.float16, device="cuda")
        wd = wt.cuda().contiguous()
        call("tsr_pack_conv_weight_f16s", ptr(wd), ptr(wp), I(cout), I(cin_), I(k), Fl(ws), stream())
        return wp, 1.0 / ws

    wp, wis = pack(w, 128, cin, ks)
    w2p, w2is = pack(w2, 64, 128, 1)
    xin = T.to_cb16(x.cuda(), cin + 16, 16)
    rbuf = T.to_cb16(res.cuda(), 80, 16) if with_res else None
    amax_in, amax_out = x.abs().max().reshape(1).cuda(), torch.zeros(1, device="cuda")
    out = torch.full((B * 96 * H * W,), float("nan"), device="cuda")
    sc, sh = scale.cuda(), shift.cuda()
    b2d = b2.cuda() if with_bias else None
    call("tsr_conv2d_fwd_f16s_fuse1x1", ptr(xin), I(cin + 16), I(16), I(cin), ptr(wp), I(ks), Fl(wis), ptr(amax_in),
         ptr(amax_out), ptr(sc), ptr(sh), I(1), ptr(w2p), Fl(w2is), ptr(b2d), ptr(rbuf), I(80 if with_res else 0),
         I(16 if with_res else 0), ptr(out), I(96), I(16), I(int(relu2)), I(B), I(H), I(W), stream())
    got = T.from_cb16(out, B, 64, H, W, 96, 16)
    err = relerr(got, ref)
    print(f"[fused 1x1] k{ks} cin{cin} B{B} {H}x{W}: {err:.2e}")
    assert err < TOL
    assert float(amax_out) == float(got.abs().max())
    assert torch.isnan(T.from_cb16(out, B, 16, H, W, 96, 0)).all() and torch.isnan(T.from_cb16(out, B, 16, H, W, 96, 80)).all()


@pytest.mark.parametrize("cin,B,H,W", [(64, 2, 40, 40), (64, 3, 13, 21), (32, 1, 100, 100), (48, 5, 8, 24), (128, 2, 16, 16)])
def test_conv2d_stage1_pair_kernel(T, cin, B, H, W):
    """tsr_conv2d_fwd_f16s_pair: conv3x3 || conv5x5 (each + folded BN + ReLU) of one input as ONE launch, output in the
    kernel's channel order (tsr_pair_channel_perm) -- against fp64 at the fp32-grade bar; ragged tiles, odd batches, one
    block pair and an odd block count (zero-padded)."""
    import ctypes
    import math
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_float as Fl
    g = torch.Generator().manual_seed(cin + 7 * B + H)
    x = torch.randn(B, cin, H, W, generator=g).clamp_(min=0) * 3
    w3 = torch.randn(64, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    w5 = torch.randn(64, cin, 5, 5, generator=g) * (2.0 / (cin * 25)) ** 0.5
    scale, shift = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.3
    ref = torch.cat([F.conv2d(x.double(), w3.double(), padding=1), F.conv2d(x.double(), w5.double(), padding=2)], 1)
    ref = F.relu(ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    arr = (ctypes.c_int * 128)()
    call("tsr_pair_channel_perm", ctypes.cast(arr, ctypes.c_void_p))
    perm = torch.tensor(list(arr))
    assert sorted(perm.tolist()) == list(range(128))
    xin = T.to_cb16(x.cuda())
    wscale = 2.0 ** (13 - math.floor(math.log2(float(max(w3.abs().max(), w5.abs().max())))))
    wp = torch.empty(load().tsr_conv_weight_pair_elems(cin), dtype=torch.float16, device="cuda")
    w3d, w5d = w3.cuda().contiguous(), w5.cuda().contiguous()        # (kept alive until the pack kernel has run)
    call("tsr_pack_conv_weight_pair_f16s", ptr(w3d), ptr(w5d), ptr(wp), I(cin), Fl(wscale), ptr(None), stream())
    torch.cuda.synchronize()
    amax_in = x.abs().max().reshape(1).cuda()
    amax_out = torch.zeros(1, device="cuda")
    out = torch.empty(B * 128 * H * W, device="cuda")
    sc, sh = scale[perm].cuda().contiguous(), shift[perm].cuda().contiguous()
    call("tsr_conv2d_fwd_f16s_pair", ptr(xin), I(cin), I(0), I(cin), ptr(wp), Fl(1.0 / wscale), ptr(amax_in),
         ptr(amax_out), ptr(sc), ptr(sh), ptr(out), I(128), I(0), I(1), I(B), I(H), I(W), stream())
    got = T.from_cb16(out, B, 128, H, W)              # kernel channel order
    err = relerr(got, ref[:, perm])
    print(f"[pair] {cin}->64||64 B={B} {H}x{W}: err vs f64 {err:.2e}")
    assert err < TOL
    assert abs(float(amax_out) - float(got.abs().max())) == 0.0


@pytest.mark.parametrize("cin,B,H,W", [(64, 5, 40, 40), (64, 2, 13, 21), (32, 1, 100, 100)])
def test_conv2d_stage1_pair_kernel_bf16_storage(T, cin, B, H, W):
    """tsr_conv2d_fwd_b16k_pair: conv3x3 || conv5x5 (+ folded BN + ReLU) of one bf16 input as ONE launch (the 3x3 half's
    outer-tap MFMAs are skipped), output = torch.cat order as a bf16 tensor.  Yardstick: fp64 convolutions of the
    bf16-ROUNDED input and weights (exact products, wide accumulation) rounded to bf16 once -- the device differs only by its
    fp32 accumulation order: >= 99 % of the elements identical, the rest within one bf16 ulp; and the result equals the
    two-launch form (tsr_conv2d_fwd_b16k twice, the 64-channel 3x3 / 5x5 instantiations) up to the same one-ulp
    rounding-boundary flips."""
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I
    g = torch.Generator().manual_seed(cin + 7 * B + H)
    x = (torch.randn(B, cin, H, W, generator=g).clamp_(min=0) * 3).bfloat16()
    w3 = torch.randn(64, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    w5 = torch.randn(64, cin, 5, 5, generator=g) * (2.0 / (cin * 25)) ** 0.5
    scale, shift = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.3
    xq, w3q, w5q = x.double(), w3.bfloat16().double(), w5.bfloat16().double()
    ref = torch.cat([F.conv2d(xq, w3q, padding=1), F.conv2d(xq, w5q, padding=2)], 1)
    ref = F.relu(ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).float().bfloat16()

    def cb16_bf16(t):        # NCHW bf16 -> CB16 bf16
        return T.to_cb16(t.float().cuda()).to(torch.bfloat16)

    def pack(w, cout, ks):
        n = load().tsr_conv_weight_b16k_elems(cout, cin, ks)
        wp = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        wd = w.cuda().contiguous()
        call("tsr_pack_conv_weight_b16k", ptr(wd), ptr(wp), I(cout), I(cin), I(ks), stream())
        torch.cuda.synchronize()
        return wp
    xin = cb16_bf16(x)
    wpair = torch.empty(load().tsr_conv_weight_b16k_pair_elems(cin), dtype=torch.bfloat16, device="cuda")
    wcat = torch.cat([F.pad(w3, (1, 1, 1, 1)), w5], 0).cuda().contiguous()
    call("tsr_pack_conv_weight_b16k_pair", ptr(wcat), ptr(wpair), I(cin), stream())
    sc, sh = scale.cuda(), shift.cuda()
    out = torch.empty(B * 128 * H * W, dtype=torch.bfloat16, device="cuda")
    call("tsr_conv2d_fwd_b16k_pair", ptr(xin), I(cin), I(0), I(cin), ptr(wpair), ptr(sc), ptr(sh), ptr(out), I(128), I(0), I(1),
         I(B), I(H), I(W), stream())
    got = T.from_cb16(out, B, 128, H, W).cpu()
    ulp = (ref.float().abs() * 2.0 ** -7).clamp_min(1e-30)
    d = (got - ref.float()).abs()
    same = float((d == 0).float().mean())
    # (near the ReLU's zero the output's own ulp is far smaller than the fp32 accumulation noise of the pre-activation:
    #  there the bar is 3e-6 of the tensor maximum)
    floor = 3e-6 * float(ref.float().abs().max())
    bad = d > torch.maximum(1.01 * ulp, torch.full_like(ulp, floor))
    print(f"[pair bf16] {cin}->64||64 B={B} {H}x{W}: identical {same:.5f}, beyond one ulp / the fp32-noise floor: {int(bad.sum())}")
    assert same >= 0.99 and not bad.any()
    # two-launch form into the two halves of the same buffer
    out2 = torch.empty_like(out)
    w3p, w5p = pack(w3, 64, 3), pack(w5, 64, 5)
    for wp_, ks, off in ((w3p, 3, 0), (w5p, 5, 64)):
        call("tsr_conv2d_fwd_b16k", ptr(xin), I(cin), I(0), I(cin), ptr(wp_), I(64), I(ks), ptr(sc[off:off + 64]),
             ptr(sh[off:off + 64]), ptr(None), I(0), I(0), ptr(out2), I(128), I(off), I(1), I(B), I(H), I(W), stream())
    got2 = T.from_cb16(out2, B, 128, H, W).cpu()
    d2 = (got - got2).abs()
    assert float((d2 == 0).float().mean()) >= 0.99 and not (d2 > torch.maximum(1.01 * ulp, torch.full_like(ulp, floor))).any()


def test_pair_and_two_launch_stage1_paths_agree(T, golden):
    """The whole eval forward with the stage-1 pair kernel (default) and with two launches per stage (the stage-2 weights
    then see their input channels in the other order)."""
    g = golden("eval")
    sd = O.random_state_dict(O.tactilesr_state_shapes(), int(g["t1/seed"]))
    m = T.TactileSR()
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    LR = torch.rand(5, 3, 4, 4, device="cuda") * 8
    m.fuse_pair = True
    y1 = m(LR)
    m.fuse_pair = False
    y0 = m(LR)
    err = relerr(y1, y0)
    print(f"[pair vs two launches] {err:.2e}")
    assert not torch.equal(y0, y1) and err < 2 * TOL      # two fp32-grade evaluations: within the sum of their bars


def test_fused_and_unfused_1x1_paths_agree(T, golden):
    """model.fuse_1x1 on/off: two fp32-grade evaluations of the same MSRB arithmetic (the fused form splits the tile with
    a tile-local scale instead of the tensor-wide one): within the sum of their 1e-5 bars."""
    g = golden("eval")
    sd = O.random_state_dict(O.tactilesr_state_shapes(), int(g["t1/seed"]))
    m = T.TactileSR()
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    LR = torch.rand(5, 3, 4, 4, device="cuda") * 8
    m.fuse_1x1 = True
    y1 = m(LR)
    m.fuse_1x1 = False
    y0 = m(LR)
    assert not torch.equal(y0, y1) and relerr(y1, y0) < 2 * TOL


@pytest.mark.parametrize("impl", ["fp16x3", "f32", "bf16x6"])
def test_tactilesrcnn_eval_forward_vs_reference_golden(golden, impl):
    """`TactileSRCNN` (reference model/tactileSR_model.py:101-153; the trainers import the name, train/tactileSR_train.py:24)
    composed from the hot path's kernels: eval forward against the reference's own output (tests/golden/srcnn.npz: its
    fp32 and fp64 runs on randomised parameters), flat 1e-5; train mode raises."""
    import tactilesr_amd
    from tactilesr_amd.model.tactileSR_model import TactileSR, TactileSRCNN   # noqa: F401  (the reference's import line)
    g = golden("srcnn")
    sd = O.random_state_dict(O.tactilesrcnn_state_shapes(), int(g["seed"]))
    m = TactileSRCNN()
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.conv_impl = impl
    x = torch.from_numpy(g["x"]).cuda()
    y = m(x)
    e32, e64 = relerr(y, torch.from_numpy(g["y"])), relerr(y, torch.from_numpy(g["y64"]))
    print(f"[TactileSRCNN {impl}] vs reference fp32 {e32:.2e}, vs reference fp64 {e64:.2e}")
    assert y.shape == (2, 1, 40, 40) and e32 < 1e-5 and e64 < 1e-5
    with torch.no_grad():                                   # in-place parameter change -> plans are rebuilt
        m.output[0].weight.mul_(0.5)
    assert relerr(m(x), torch.from_numpy(g["y"]) * 0.5) < 1e-5
    m.train()
    with pytest.raises(tactilesr_amd._lib.TactileSRHipError, match="train mode is not on the MI355X path"):
        m(x)
