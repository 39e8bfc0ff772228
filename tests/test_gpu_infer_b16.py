"""Kernel-level tests of the bf16-storage INFERENCE conv launches, ONE LAUNCH AT A TIME: tsr_conv2d_fwd_b16,
tsr_conv2d_fwd_b16k, tsr_conv2d_fwd_b16k_pair, tsr_conv2d_fwd_b16k_fuse1x1 and the pack routines behind them -- what
`conv_impl = "bf16"` runs in eval mode (csrc/conv_b16k.hip, csrc/conv_mfma_split16.hip).

The case tables with the reason of every case, the launch geometry, the yardstick and the bar are in tests/_infer_b16.py
(checked without a GPU by tests/test_infer_b16_cpu.py).  In short: every launch runs on NaN-filled bf16 buffers 48 channels
wider than the slice, with input, output and residual at three different non-zero channel offsets; every output element is
compared with fp64 on the bf16-rounded operands, rounded to bf16 once (one bf16 ulp or 3e-6 of the IMAGE's maximum, >= 99 %
bit-identical; fuse1x1: two ulps or 2e-3, >= 98 %; a failure names the image, 8x8 tile and 16-channel block), and everything
outside the output slice must still be NaN.

  1. test_b16_one_launch, test_b16k_one_launch, test_b16k_pair_one_launch, test_b16k_fuse1x1_one_launch over the tables: scale /
     shift / res each NULL or not, relu 0 / 1, all eight (shift2, res, relu2)
  2. test_pack_*                     the packed weights against their documented layout, bit for bit
  3. cross-form identities           pair == the two b16k launches it replaces; the model's fuse1x1 chain (P from the 3x3 launch,
                                     out from the 5x5 launch with res = P) == `confusion` over cat([stage 3x3, stage 5x5]); b16 and
                                     b16k meet the same bar against the same reference
  4. test_non_finite_*               a NaN / +Inf pixel of image 1 reaches its ks x ks window in image 1 and nothing else: every
                                     other output is finite and bit-identical to the clean run
  5. refusals                        every mutation of _infer_b16.mutations returns 1 and leaves the NaN-filled output as it was;
                                     the unmodified list then returns 0 and meets the bar (also tsr_conv2d_fwd, _bf16s, _ex with
                                     their negative offsets, and the pack routines on a sentinel-filled buffer)

Measured on an MI355X, lowest bit-identical share over the cases of a launch kind (nothing beyond the bar anywhere):
    tsr_conv2d_fwd_b16            0.99974   (5x5 48 -> 128, B = 2, 5x3: 1 of 3840 elements; the 448-channel case: 1.00000)
    tsr_conv2d_fwd_b16k           0.99965   (5x5 96 -> 128, B = 3, 5x3: 2 of 5760)
    tsr_conv2d_fwd_b16k_pair      0.99971   (C_in 128, B = 5, 9x17: 28 of 97920); pair vs its two launches: 1.00000
    tsr_conv2d_fwd_b16k_fuse1x1   0.99937   (5x5 C_in 32, B = 1, 13x21: 11 of 17472); model chain: P 0.99991, out 0.99969
"""
import pytest
import torch
import torch.nn.functional as F

import _infer_b16 as S
import _infer_f16s as S32
from _infer_b16 import PAD, NAN, BAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


def dev(t):
    return None if t is None else t.cuda().contiguous()


def stream():
    from tactilesr_amd._lib import stream as st
    return st()


def launch(kind, vals):
    st = S.raw(kind, vals, stream())
    assert st == 0, f"{S.SIGS[kind][0]}: status {st}"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- launches
def conv_args(kind, p, offs, packed=None):
    """Argument list of tsr_conv2d_fwd_b16 (kind "b16") / tsr_conv2d_fwd_b16k ("b16k")."""
    x, w = p["x"], p["w"]
    B, cin, H, W = x.shape
    cout, ks = w.shape[0], w.shape[2]
    wp = packed if packed is not None else (S.pack_b16(w) if kind == "b16" else S.pack_b16k(w))
    res = p.get("res")
    return {"in": S.slice_buffer_b16(x, offs[0]), "in_ctot": cin + PAD, "in_coff": offs[0], "cin": cin, "w_packed": wp, "cout": cout,
            "ks": ks, "scale": dev(p.get("scale")), "shift": dev(p.get("shift")),
            "res": None if res is None else S.slice_buffer_b16(res, offs[2]), "res_ctot": 0 if res is None else cout + PAD,
            "res_coff": 0 if res is None else offs[2], "out": S.nan_output_b16(B, cout, H, W), "out_ctot": cout + PAD,
            "out_coff": offs[1], "relu": int(p.get("relu", 0)), "B": B, "H": H, "W": W}


def run_conv(kind, p, offs, packed=None):
    a = conv_args(kind, p, offs, packed)
    launch(kind, a)
    return S.read_slice_b16(a["out"], a["B"], a["cout"], a["H"], a["W"], offs[1])[0]


def pair_args(p, offs):
    x = p["x"]
    B, cin, H, W = x.shape
    return {"in": S.slice_buffer_b16(x, offs[0]), "in_ctot": cin + PAD, "in_coff": offs[0], "cin": cin,
            "w_packed": S.pack_pair_b16k(p["w3"], p["w5"]), "scale": dev(p.get("scale")), "shift": dev(p.get("shift")),
            "out": S.nan_output_b16(B, 128, H, W), "out_ctot": 128 + PAD, "out_coff": offs[1], "relu": int(p.get("relu", 0)),
            "B": B, "H": H, "W": W}


def run_pair(p, offs):
    a = pair_args(p, offs)
    launch("pair", a)
    return S.read_slice_b16(a["out"], a["B"], 128, a["H"], a["W"], offs[1])[0]


def fuse_args(p, offs):
    x, w = p["x"], p["w"]
    B, cin, H, W = x.shape
    res = p.get("res")
    return {"in": S.slice_buffer_b16(x, offs[0]), "in_ctot": cin + PAD, "in_coff": offs[0], "cin": cin, "w_packed": S.pack_b16k(w),
            "ks": w.shape[2], "scale": dev(p.get("scale")), "shift": dev(p.get("shift")), "relu": int(p.get("relu", 0)),
            "w2_packed": S.pack_w2_b16k(p["w2"]), "shift2": dev(p.get("shift2")),
            "res": None if res is None else S.slice_buffer_b16(res, offs[2]), "res_ctot": 0 if res is None else 64 + PAD,
            "res_coff": 0 if res is None else offs[2], "out": S.nan_output_b16(B, 64, H, W), "out_ctot": 64 + PAD,
            "out_coff": offs[1], "relu2": int(p.get("relu2", 0)), "B": B, "H": H, "W": W}


def run_fuse(p, offs):
    a = fuse_args(p, offs)
    launch("fuse1x1", a)
    return S.read_slice_b16(a["out"], a["B"], 64, a["H"], a["W"], offs[1])[0]


RUN = {"b16": lambda p, o: run_conv("b16", p, o), "b16k": lambda p, o: run_conv("b16k", p, o), "pair": run_pair, "fuse1x1": run_fuse}


def one_launch(kind, c):
    inputs, ref_fn = S.INPUTS[kind]
    p = inputs(c)
    ref = ref_fn(p)
    assert S.image_ratio(ref) < 4
    got = RUN[kind](p, c.offs)
    try:
        same, off = S.check_elements(got, ref, *BAR[kind])
    except S.ElementMismatch as e:
        print(f"[{kind}] {S.cid(c)} grid {S.case_grid(kind, c)}: {e}")
        raise
    print(f"[{kind}] {S.cid(c)} grid {S.case_grid(kind, c)}: identical {same:.5f}, {off} of {got.numel()} elements differ (all within "
          f"the bar), image max ratio {S.image_ratio(ref):.2f}")


# ------------------------------------------------------------------------------------------- 1. one launch at a time
@pytest.mark.parametrize("case", S.B16_CASES, ids=S.cid)
def test_b16_one_launch(T, case):
    """tsr_conv2d_fwd_b16: out slice == bf16(act(conv(x slice) * scale + shift + res slice)) element by element, scale / shift /
    res independently NULL, nothing outside the output slice written."""
    one_launch("b16", case)


@pytest.mark.parametrize("case", S.B16K_CASES, ids=S.cid)
def test_b16k_one_launch(T, case):
    """tsr_conv2d_fwd_b16k (B16K_PLAIN): every path of b16k_epilogue's plain form -- ReLU or not, residual or not, NULL scale /
    shift -- and every slot phase of the circular halo buffer."""
    one_launch("b16k", case)


@pytest.mark.parametrize("case", S.PAIR_CASES, ids=S.cid)
def test_b16k_pair_one_launch(T, case):
    """tsr_conv2d_fwd_b16k_pair (B16K_PAIR): conv3x3 || conv5x5 of one input slice, output in torch.cat order."""
    one_launch("pair", case)


@pytest.mark.parametrize("case", S.FUSE_CASES, ids=S.cid)
def test_b16k_fuse1x1_one_launch(T, case):
    """tsr_conv2d_fwd_b16k_fuse1x1 (B16K_FUSED): act2(w2 . act(conv(x) * scale + shift) + shift2 + res), res and out in different
    slices, all eight (shift2, res, relu2)."""
    one_launch("fuse1x1", case)


# ------------------------------------------------------------------------------------------- 2. pack routines, bit for bit
def bits(t):
    return t.cpu().contiguous().view(torch.int16)


@pytest.mark.parametrize("cout,cin,ks", [(64, 32, 3), (128, 96, 5), (64, 64, 1)])
def test_pack_conv_weight_b16k_layout(T, cout, cin, ks):
    """Element [cb][tap][g][co][j] == bf16(w[co][cb * 32 + g * 8 + j][tap])."""
    g = torch.Generator().manual_seed(cout + cin + ks)
    w = S.he(g, cout, cin, ks)
    wp = S.pack_b16k(w)
    want = w.bfloat16().view(cout, cin // 32, 4, 8, ks * ks).permute(1, 4, 2, 0, 3).contiguous()       # [cb][tap][g][co][j]
    assert wp.numel() == want.numel() == cout * cin * ks * ks
    assert torch.equal(bits(wp), bits(want.reshape(-1)))


def test_pack_w2_b16k_layout(T):
    """Element [kk][g][co][j] == bf16(0.5 * w2[co][ch]), ch = 32 kk + (j < 4 ? 4 g + j : 16 + 4 g + j - 4)."""
    g = torch.Generator().manual_seed(5)
    w2 = torch.randn(64, 128, generator=g) * 0.1
    wp = S.pack_w2_b16k(w2)
    kk, gg, co, j = torch.meshgrid(torch.arange(4), torch.arange(4), torch.arange(64), torch.arange(8), indexing="ij")
    ch = 32 * kk + torch.where(j < 4, 4 * gg + j, 16 + 4 * gg + j - 4)
    want = (0.5 * w2)[co, ch].bfloat16()
    assert sorted(ch[:, :, 0].reshape(-1).tolist()) == list(range(128))
    assert torch.equal(bits(wp), bits(want.reshape(-1)))


def pair_steps():
    """The barrier steps of a channel block of the pair form (B16KSteps<5, B16K_PAIR>): [(first tap, taps)] -- two consecutive
    outer taps share a step."""
    def outer(t):
        return not (1 <= t // 5 <= 3 and 1 <= t % 5 <= 3)
    steps, t = [], 0
    while t < 25:
        n = 2 if outer(t) and t + 1 < 25 and outer(t + 1) else 1
        steps.append((t, n))
        t += n
    return steps


@pytest.mark.parametrize("cin", [32, 96])
def test_pack_conv_weight_b16k_pair_layout(T, cin):
    """The packed stage-1 pair is a permutation of bf16(W) restricted to the taps each conv owns (the 128 x C_in x 9 inner-tap
    weights + the 64 x C_in x 16 outer-tap weights of the 5x5 half), in the documented order: one [g 4][row 128][j 8] slab per
    barrier step; an inner tap's slab holds all 128 channels, a double step (u, u + 1) the 5x5 conv's 64 channels at tap u + 1
    (rows 0..63) and at tap u (rows 64..127)."""
    g = torch.Generator().manual_seed(cin)
    w3, w5 = S.he(g, 64, cin, 3), S.he(g, 64, cin, 5)
    wp = S.pack_pair_b16k(w3, w5)
    wc = S.pair_weight(w3, w5).bfloat16().view(128, cin, 25)
    steps = pair_steps()
    assert len(steps) == 17 and sum(n for _, n in steps) == 25 and sum(n == 2 for _, n in steps) == 8
    inner = [t for t, n in steps if n == 1]
    outer = [t + i for t, n in steps if n == 2 for i in range(2)]
    multiset = torch.cat([wc[:, :, inner].reshape(-1), wc[64:, :, outer].reshape(-1)])
    assert wp.numel() == multiset.numel() == (cin // 32) * 17 * 4096
    assert torch.equal(bits(wp).sort().values, bits(multiset).sort().values)
    assert float(wc[:64, :, outer].abs().max()) == 0                       # (the 3x3 half owns nothing on the outer taps)
    want = torch.empty(cin // 32, 17, 4, 128, 8, dtype=torch.bfloat16)
    for s, (t0, n) in enumerate(steps):
        blk = wc.view(128, cin // 32, 4, 8, 25)
        if n == 1:
            want[:, s] = blk[..., t0].permute(1, 2, 0, 3)
        else:
            want[:, s, :, :64] = blk[64:, ..., t0 + 1].permute(1, 2, 0, 3)
            want[:, s, :, 64:] = blk[64:, ..., t0].permute(1, 2, 0, 3)
    assert torch.equal(bits(wp), bits(want.reshape(-1)))


# ------------------------------------------------------------------------------------------- 3. cross-form identities
@pytest.mark.parametrize("cin,relu", [(32, 0), (32, 1), (96, 0), (96, 1)])
def test_pair_equals_the_two_launches_it_replaces(T, cin, relu):
    """The pair launch against two tsr_conv2d_fwd_b16k launches (the 64-channel 3x3 and 5x5 instances) into the two halves of
    one slice: two fp32 evaluations of the same sums -- identical up to one-ulp rounding-boundary flips (the pair's bar)."""
    c = S.PairCase(cin, 3, 13, 21, True, True, relu, (16, 32))
    p = S.pair_inputs(c, seed=1)
    got = run_pair(p, c.offs)
    out = S.nan_output_b16(c.B, 128, c.H, c.W)
    for w, off in ((p["w3"], 0), (p["w5"], 64)):
        a = conv_args("b16k", dict(x=p["x"], w=w, scale=p["scale"][off:off + 64], shift=p["shift"][off:off + 64], relu=relu), (48, 0, 0))
        a.update(out=out, out_ctot=128 + PAD, out_coff=32 + off)
        launch("b16k", a)
    two, _ = S.read_slice_b16(out, c.B, 128, c.H, c.W, 32)
    same, off = S.check_elements(got, two, *BAR["pair"])
    ref = S.pair_ref(p)
    s1, _ = S.check_elements(got, ref, *BAR["pair"])
    s2, _ = S.check_elements(two, ref, *BAR["b16k"])
    print(f"[pair vs two launches] C_in {cin} relu {relu}: identical {same:.5f} ({off} differ); against fp64: pair {s1:.5f}, two {s2:.5f}")


def test_fuse1x1_model_chain(T):
    """The two launches the model issues for MSRB stage 2 + `confusion`: P = W_a . stage3(x1) + b_c + x (3x3 launch, relu2 = 0),
    out = relu(W_b . stage5(x1) + P) (5x5 launch, res = P read from the slice the first launch wrote), against fp64 `confusion`
    over cat([stage 3x3, stage 5x5]) + b_c + x with the stage tiles rounded to bf16 (the B operand of the 1x1 product) and bf16
    rounding at the two stored tensors, P and out.  B = 2, 13x21, the fuse1x1 bar."""
    B, H, W = 2, 13, 21
    g = torch.Generator().manual_seed(77)
    x1 = torch.randn(B, 128, H, W, generator=g) * 3
    x = torch.randn(B, 64, H, W, generator=g) * 3
    wc = torch.randn(64, 256, generator=g) * (2.0 / 256) ** 0.5                        # `confusion`: [W_a | W_b]
    bc = torch.randn(64, generator=g) * 0.2
    pa = dict(x=x1, w=S.he(g, 128, 128, 3), scale=torch.rand(128, generator=g) + 0.5, shift=torch.randn(128, generator=g) * 0.3,
              relu=1, w2=wc[:, :128].contiguous(), shift2=bc, res=x, relu2=0)
    pb = dict(x=x1, w=S.he(g, 128, 128, 5), scale=torch.rand(128, generator=g) + 0.5, shift=torch.randn(128, generator=g) * 0.3,
              relu=1, w2=wc[:, 128:].contiguous(), shift2=None, res=None, relu2=1)
    s3 = S.round_b16(S.ref_conv(S.q16(x1), S.q16(pa["w"]), pa["scale"], pa["shift"], None, 1)).double()
    s5 = S.round_b16(S.ref_conv(S.q16(x1), S.q16(pb["w"]), pb["scale"], pb["shift"], None, 1)).double()
    wq = S.q16(wc).double()
    refP = S.round_b16(torch.einsum("oc,bchw->bohw", wq[:, :128], s3) + bc.double().view(1, -1, 1, 1) + S.q16(x).double())
    ref = S.round_b16(F.relu(torch.einsum("oc,bchw->bohw", wq[:, 128:], s5) + refP.double()))
    whole = F.relu(torch.einsum("oc,bchw->bohw", wq, torch.cat([s3, s5], 1)) + bc.double().view(1, -1, 1, 1) + S.q16(x).double())
    assert float((ref.double() - whole).abs().max()) <= 2.0 ** -7 * float(whole.abs().max())       # (one composition, P's rounding apart)
    assert S.image_ratio(refP) < 4 and S.image_ratio(ref) < 4
    a = fuse_args(pa, (16, 32, 48))
    launch("fuse1x1", a)
    P, _ = S.read_slice_b16(a["out"], B, 64, H, W, 32)
    sP, oP = S.check_elements(P, refP, *BAR["fuse1x1"])
    b = fuse_args(pb, (48, 16, 0))
    b.update(res=a["out"], res_ctot=64 + PAD, res_coff=32)               # P where the first launch left it
    launch("fuse1x1", b)
    out, _ = S.read_slice_b16(b["out"], B, 64, H, W, 16)
    s, o = S.check_elements(out, ref, *BAR["fuse1x1"])
    print(f"[fuse1x1 chain] P identical {sP:.5f} ({oP} differ); out identical {s:.5f} ({o} differ)")


def test_b16_and_b16k_agree(T):
    """3x3 128 -> 128, B = 3, 13x21, with residual: both kernels meet the one-ulp bar against the same reference."""
    c = S.B16Case(3, 128, 128, 3, 13, 21, True, True, True, 1, (16, 32, 48))
    p = S.b16_inputs(c, seed=2)
    ref = S.b16_ref(p)
    a = run_conv("b16", p, c.offs)
    b = run_conv("b16k", p, (48, 16, 32))
    sa, oa = S.check_elements(a, ref, *BAR["b16"])
    sb, ob = S.check_elements(b, ref, *BAR["b16k"])
    d = int((a != b).sum())
    print(f"[b16 vs b16k] b16 identical {sa:.5f} ({oa} differ), b16k {sb:.5f} ({ob} differ); {d} elements differ between the two")
    assert d <= oa + ob


# ------------------------------------------------------------------------------------------- 4. non-finite input
NF_B, NF_H, NF_W, NF_Y, NF_X, NF_CH = 5, 13, 21, 7, 8, 37          # the pixel sits on a tile corner: its window spans four tiles


def nf_launches():
    return [("b16k", 3, 64, 128), ("b16k", 5, 64, 64), ("pair", 5, 64, 128), ("b16", 3, 64, 64)]


@pytest.mark.parametrize("bad", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("kind,ks,cin,cout", nf_launches(), ids=lambda v: str(v))
def test_non_finite_input_stays_in_its_receptive_field(T, kind, ks, cin, cout, bad):
    """One non-finite element at (image 1, channel 37, y 7, x 8), no residual, no ReLU: outside that pixel's ks x ks window of
    image 1 and in images 0, 2, 3, 4 -- which share the workgroup's LDS ring with image 1 -- every output is finite and
    bit-identical to the clean run; inside the window a NaN input gives NaN in every channel (pair: 3x3 window for the 3x3 half)."""
    if kind == "pair":
        c = S.PairCase(cin, NF_B, NF_H, NF_W, True, True, 0, (16, 32))
        p, run = S.pair_inputs(c, seed=3), run_pair
    else:
        c = S.B16Case(ks, cin, cout, NF_B, NF_H, NF_W, True, True, False, 0, (32, 48, 16))
        p, run = S.b16_inputs(c, seed=3), RUN[kind]
    clean = run(p, c.offs)
    assert torch.isfinite(clean).all()
    x = p["x"].clone()
    x[1, NF_CH, NF_Y, NF_X] = bad
    got = run(dict(p, x=x), c.offs)
    inside = torch.zeros_like(clean, dtype=torch.bool)
    r = ks // 2
    inside[1, :, NF_Y - r:NF_Y + r + 1, NF_X - r:NF_X + r + 1] = True
    if kind == "pair":
        inside[1, :64] = False
        inside[1, :64, NF_Y - 1:NF_Y + 2, NF_X - 1:NF_X + 2] = True
    out = ~inside
    assert torch.isfinite(got[out]).all(), "a non-finite input left its receptive field"
    assert torch.equal(got[out].view(torch.int32), clean[out].view(torch.int32)), "an output outside the window changed"
    if bad != bad:
        assert torch.isnan(got[inside]).all(), "a NaN input did not reach its whole window"
    else:
        assert not torch.isfinite(got[inside]).all()


# ------------------------------------------------------------------------------------------- 5. refusals
def check_refusals(kind, args, width, ref):
    """Every mutated argument list returns 1 and launches nothing; the unmodified one returns 0 and meets the bar."""
    muts = S.mutations(kind)
    for name, m in muts:
        st = S.raw(kind, dict(args, **m), stream())
        assert st == 1, f"{S.SIGS[kind][0]} with {name}: status {st}"
    torch.cuda.synchronize()
    assert torch.isnan(args["out"]).all(), "a refused call wrote the output"
    launch(kind, args)
    got, _ = S.read_slice_b16(args["out"], args["B"], width, args["H"], args["W"], args["out_coff"])
    S.check_elements(got, ref, *BAR[kind])
    print(f"[refusals] {S.SIGS[kind][0]}: {len(muts)} argument lists refused")


@pytest.mark.parametrize("kind", ["b16", "b16k", "pair", "fuse1x1"])
def test_refusals(T, kind):
    c = S.REFUSAL_CASES[kind]
    inputs, ref_fn = S.INPUTS[kind]
    p = inputs(c)
    a = {"pair": pair_args, "fuse1x1": fuse_args}.get(kind, lambda p_, o: conv_args(kind, p_, o))(p, c.offs)
    ints = S.valid_ints(kind)
    assert {k: a[k] for k in ints} == ints, "the GPU test's valid list is the CPU test's"
    check_refusals(kind, a, S.OUT_WIDTH.get(kind) or c.cout, ref_fn(p))


@pytest.mark.parametrize("kind", ["f32", "bf16s", "ex"])
def test_fp32_launches_refuse_negative_offsets(T, kind):
    """tsr_conv2d_fwd, tsr_conv2d_fwd_bf16s (nsplit 3) and tsr_conv2d_ex (nsplit 0, epi_mode 0) on fp32 CB16 buffers: the
    negative-offset mutations return 1 and write nothing; the valid 3x3 64 -> 64, B = 1, 8x8 list returns 0 at TOL = 1e-5."""
    from tactilesr_amd import _lib as L
    c = S.REFUSAL_CASES[kind]
    p = S32.f16s_inputs(S32.F16sCase(*c[:10], None, c.offs))
    ref = S32.f16s_ref(p)
    wd = dev(p["w"])
    if kind == "bf16s":
        wp = torch.zeros(L.load().tsr_conv_weight_bf16s_elems(c.cout, c.cin, c.ks, 3), dtype=torch.bfloat16, device="cuda")
        L.call("tsr_pack_conv_weight_bf16s", L.ptr(wd), L.ptr(wp), L.c_int(c.cout), L.c_int(c.cin), L.c_int(c.ks), L.c_int(3), L.stream())
    else:
        wp = torch.zeros(c.cout * c.cin * c.ks * c.ks, device="cuda")
        L.call("tsr_pack_conv_weight", L.ptr(wd), L.ptr(wp), L.c_int(c.cout), L.c_int(c.cin), L.c_int(c.ks), L.stream())
    torch.cuda.synchronize()
    a = dict(S.valid_ints(kind))
    a.update({"in": S32.slice_buffer(p["x"], c.offs[0]), "w_packed": wp, "scale": dev(p["scale"]), "shift": dev(p["shift"]),
              "res": S32.slice_buffer(p["res"], c.offs[2]), "out": S32.nan_output(c.B, c.cout, c.H, c.W)})
    call = (lambda v: S.raw_ex(v, stream())) if kind == "ex" else (lambda v: S.raw(kind, v, stream()))
    for name, m in S.mutations(kind):
        assert call(dict(a, **m)) == 1, f"{kind} with {name}"
    torch.cuda.synchronize()
    assert torch.isnan(a["out"]).all(), "a refused call wrote the output"
    assert call(a) == 0
    torch.cuda.synchronize()
    got, _ = S32.read_slice(a["out"], c.B, c.cout, c.H, c.W, c.offs[1])
    S32.check_images(got, ref, S32.TOL)


def test_pack_refusals(T):
    """Every pack routine: a refused call leaves the sentinel-filled buffer as it was; the valid call then writes it."""
    from tactilesr_amd._lib import load
    SENT = 0x7A7A
    g = torch.Generator().manual_seed(9)
    n = 0
    for kind in ("pack_f32", "pack_bf16s", "pack_b16k", "pack_pair", "pack_w2"):
        ints, muts = S.pack_mutations(kind)
        if kind == "pack_w2":
            w, elems = torch.randn(64, 128, generator=g) * 0.1, 64 * 128
        elif kind == "pack_pair":
            w, elems = S.pair_weight(S.he(g, 64, 32, 3), S.he(g, 64, 32, 5)), load().tsr_conv_weight_b16k_pair_elems(32)
        else:
            cout, cin, ks = ints["cout"], ints["cin"], ints["ks"]
            w = S.he(g, cout, cin, ks)
            elems = {"pack_f32": 2 * w.numel(),                              # (fp32 elements: two 16-bit words each)
                     "pack_bf16s": load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 1),
                     "pack_b16k": load().tsr_conv_weight_b16k_elems(cout, cin, ks)}[kind]
            assert elems >= w.numel()
        buf = torch.full((elems,), SENT, dtype=torch.int16, device="cuda")
        base = dict(ints, w=dev(w), w_packed=buf)
        for name, m in muts:
            assert S.raw(kind, dict(base, **m), stream()) == 1, f"{S.SIGS[kind][0]} with {name}"
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), f"a refused {S.SIGS[kind][0]} wrote its buffer"
        assert S.raw(kind, base, stream()) == 0
        torch.cuda.synchronize()
        # (the buffer may be larger than the weight -- padded taps / channel blocks -- or smaller: the pair drops the zero taps)
        assert int((buf != SENT).sum()) >= 0.99 * min(elems, w.numel()), S.SIGS[kind][0]
        n += len(muts)
    print(f"[refusals] pack routines: {n} argument lists refused")
