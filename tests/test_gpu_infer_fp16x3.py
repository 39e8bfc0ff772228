"""Kernel-level tests of the fp16x3 INFERENCE conv launches, ONE LAUNCH AT A TIME: tsr_conv2d_fwd_f16s,
tsr_conv2d_fwd_f16s_pair, tsr_conv2d_fwd_f16s_fuse1x1 and the four pack routines behind them -- what `TactileSR` and
`TactileSRCNN` run by default in eval mode (`conv_impl = "fp16x3"`).  The train step's launches have tests/test_gpu_conv_ex.py;
these are distinct template instances (`EXT = false`), and the pair and fuse1x1 forms have no train twin.

The case tables with the reason of every case, the launch geometry and the bar are in tests/_infer_f16s.py (checked without a
GPU by tests/test_infer_f16s_cpu.py).  In short: every launch runs on NaN-filled buffers 48 channels wider than the slice, with
input, output and residual at three different non-zero channel offsets; every output element is compared with fp64 on the fp32
operands at TOL = 1e-5 PER IMAGE (the failure names the image, 8x8 tile and 16-channel block), and everything outside the
output slice must still be NaN.

  1. test_f16s_one_launch            F16S_CASES: scale / shift / res each NULL or not, relu 0 / 1, the four out_amax settings
  2. test_pack_dev_*                 device-side weight scale == host-side weight scale, bit for bit (3x3, 5x5, 1x1, pair)
  3. test_pair_one_launch            PAIR_CASES in tsr_pair_channel_perm order;  test_pair_3x3_half_equals_single_launch: 2 TOL
  4. test_fuse1x1_one_launch         FUSE_CASES (all eight (shift2, res, relu2));  test_fuse1x1_model_chain: the two launches
                                     the model issues (3x3: w2 = W_a, shift2 = b_c, res = x; 5x5: w2 = W_b, res = P, relu2)
  5. the scale contract (include/tactilesr_hip.h, "in_amax / out_amax"), on a 3x3 K = 32 launch, a 1x1 launch, a pair launch and
     a fuse1x1 launch at 13x21, B = 3:
       same binade       in_amax = max|x| and the largest float of its binade: bit-identical outputs and out_amax
       homogeneity       x * 2^k with in_amax * 2^k, k in {-60, -20, +20, +60}, power-of-two `scale`, no shift / residual:
                         exactly 2^k times the k = 0 output and out_amax (every scale is a power of two, undone exactly)
       loose bound       in_amax = 2^j max|x| costs j bits of the activation planes: error < 2^j TOL per image, j = 0, 1, 2
       zero input        x = 0, in_amax = 0: exactly act(shift + res) (fuse1x1: the fp64 reference on a zero input at TOL)
  6. refusals            every argument check of the three launches and the pack routines returns 1 and launches nothing:
                         the NaN-filled output and a preset out_amax (a sentinel-filled pack buffer) are unchanged after a
                         synchronize; the unmodified argument list then returns 0 and passes the bar
"""
import ctypes
import math

import pytest
import torch

import _infer_f16s as S
from _infer_f16s import PAD, TOL, F16S_SIG, PAIR_SIG, FUSE_SIG, PACK_SIG, PACK_DEV_SIG, PACK_PAIR_SIG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


def dev(t):
    return None if t is None else t.cuda().contiguous()


def f32(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


# ---------------------------------------------------------------------------------------------------------------- launches
def raw(name, sig, vals):
    """The entry point's status for the argument list `vals` (name -> tensor / None / int / float), no exception."""
    from tactilesr_amd._lib import load, ptr, stream, c_int, c_float
    args = []
    for s in sig:
        n, t = s.split(":")
        args.append(ptr(vals[n]) if t == "p" else (c_int(vals[n]) if t == "i" else c_float(vals[n])))
    return getattr(load(), name)(*args, stream())


def launch(name, sig, vals):
    st = raw(name, sig, vals)
    assert st == 0, f"{name}: status {st}"
    torch.cuda.synchronize()


def f16s_args(p, offs, in_amax=None, prior=None, packed=None):
    x, w = p["x"], p["w"]
    B, cin, H, W = x.shape
    cout, ks = w.shape[0], w.shape[2]
    wp, inv = S.pack_f16s(w) if packed is None else packed
    res = p.get("res")
    return {"in": S.slice_buffer(x, offs[0]), "in_ctot": cin + PAD, "in_coff": offs[0], "cin": cin, "w_packed": wp, "cout": cout,
            "ks": ks, "w_inv_scale": inv, "in_amax": f32(float(x.abs().max()) if in_amax is None else in_amax),
            "out_amax": None if prior is None else f32(prior), "scale": dev(p.get("scale")), "shift": dev(p.get("shift")),
            "res": None if res is None else S.slice_buffer(res, offs[2]), "res_ctot": 0 if res is None else cout + PAD,
            "res_coff": 0 if res is None else offs[2], "out": S.nan_output(B, cout, H, W), "out_ctot": cout + PAD,
            "out_coff": offs[1], "relu": int(p.get("relu", 0)), "B": B, "H": H, "W": W}


def run_f16s(p, offs, in_amax=None, prior=None, packed=None):
    """One tsr_conv2d_fwd_f16s launch -> (output slice as NCHW on the CPU, out_amax tensor or None)."""
    a = f16s_args(p, offs, in_amax, prior, packed)
    launch("tsr_conv2d_fwd_f16s", F16S_SIG, a)
    got, _ = S.read_slice(a["out"], a["B"], a["cout"], a["H"], a["W"], offs[1])
    return got, a["out_amax"]


def pair_args(p, offs, in_amax=None, prior=None, packed=None):
    x = p["x"]
    B, cin, H, W = x.shape
    wp, inv = S.pack_pair(p["w3"], p["w5"]) if packed is None else packed
    return {"in": S.slice_buffer(x, offs[0]), "in_ctot": cin + PAD, "in_coff": offs[0], "cin": cin, "w_packed": wp,
            "w_inv_scale": inv, "in_amax": f32(float(x.abs().max()) if in_amax is None else in_amax),
            "out_amax": None if prior is None else f32(prior), "scale": dev(p.get("scale")), "shift": dev(p.get("shift")),
            "out": S.nan_output(B, 128, H, W), "out_ctot": 128 + PAD, "out_coff": offs[1], "relu": int(p.get("relu", 0)),
            "B": B, "H": H, "W": W}


def run_pair(p, offs, in_amax=None, prior=None, packed=None):
    a = pair_args(p, offs, in_amax, prior, packed)
    launch("tsr_conv2d_fwd_f16s_pair", PAIR_SIG, a)
    got, _ = S.read_slice(a["out"], a["B"], 128, a["H"], a["W"], offs[1])
    return got, a["out_amax"]


def fuse_args(p, offs, in_amax=None, prior=None, packed=None):
    x, w = p["x"], p["w"]
    B, cin, H, W = x.shape
    wp, inv = S.pack_f16s(w) if packed is None else packed
    w2p, inv2 = S.pack_w2(p["w2"])
    res = p.get("res")
    return {"in": S.slice_buffer(x, offs[0]), "in_ctot": cin + PAD, "in_coff": offs[0], "cin": cin, "w_packed": wp,
            "ks": w.shape[2], "w_inv_scale": inv, "in_amax": f32(float(x.abs().max()) if in_amax is None else in_amax),
            "out_amax": None if prior is None else f32(prior), "scale": dev(p.get("scale")), "shift": dev(p.get("shift")),
            "relu": int(p.get("relu", 0)), "w2_packed": w2p, "w2_inv_scale": inv2, "shift2": dev(p.get("shift2")),
            "res": None if res is None else S.slice_buffer(res, offs[2]), "res_ctot": 0 if res is None else 64 + PAD,
            "res_coff": 0 if res is None else offs[2], "out": S.nan_output(B, 64, H, W), "out_ctot": 64 + PAD,
            "out_coff": offs[1], "relu2": int(p.get("relu2", 0)), "B": B, "H": H, "W": W}


def run_fuse(p, offs, in_amax=None, prior=None, packed=None):
    a = fuse_args(p, offs, in_amax, prior, packed)
    launch("tsr_conv2d_fwd_f16s_fuse1x1", FUSE_SIG, a)
    got, _ = S.read_slice(a["out"], a["B"], 64, a["H"], a["W"], offs[1])
    return got, a["out_amax"]


def one_launch(tag, c, inputs, ref_fn, run):
    p = inputs(c)
    ref = ref_fn(p)
    assert S.image_ratio(ref) < 4
    prior = S.amax_prior(c.amax, ref)
    got, am = run(p, c.offs, prior=prior)
    per = S.check_images(got, ref, TOL)
    print(f"[{tag}] {S.cid(c)} grid {S.case_grid(c)}: {S.fmt_images(per)}, image max ratio {S.image_ratio(ref):.2f}, out_amax {c.amax}")
    assert (am is None) == (c.amax is None)
    S.check_amax(c.amax, prior, am, got)


# ------------------------------------------------------------------------------------------- 1. tsr_conv2d_fwd_f16s
@pytest.mark.parametrize("case", S.F16S_CASES, ids=S.cid)
def test_f16s_one_launch(T, case):
    """out slice == act(conv(x slice) * scale + shift + res slice) per image, scale / shift / res independently NULL, the
    out_amax slot only ever raised, nothing outside the output slice written."""
    one_launch("f16s", case, S.f16s_inputs, S.f16s_ref, run_f16s)


# ------------------------------------------------------------------------------------------- 2. device-side weight scale
@pytest.mark.parametrize("cout,cin,ks", [(64, 64, 3), (128, 48, 5), (64, 256, 1), (64, 128, 1)])
def test_pack_dev_equals_host_scale(T, cout, cin, ks):
    """tsr_pack_conv_weight_f16s_dev from a device w_amax == tsr_pack_conv_weight_f16s with the host-derived wscale, bit for
    bit (the last shape is the 1x1 half the fuse1x1 launch takes)."""
    g = torch.Generator().manual_seed(cout + cin + ks)
    w = S.he(g, cout, cin, ks)
    a, _ = S.pack_f16s(w)
    b = S.pack_f16s_dev(w)
    assert a.numel() == b.numel() and torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert float(a.float().abs().max()) >= 2.0 ** 13            # (both were written: max|w| * wscale lies in [2^13, 2^14))


@pytest.mark.parametrize("cin", [16, 64])
def test_pack_dev_equals_host_scale_pair(T, cin):
    """tsr_pack_conv_weight_pair_f16s with w_amax = max(max|w3|, max|w5|) == the same routine with the host wscale."""
    g = torch.Generator().manual_seed(cin)
    w3, w5 = S.he(g, 64, cin, 3), S.he(g, 64, cin, 5)
    a, _ = S.pack_pair(w3, w5)
    b, _ = S.pack_pair(w3, w5, dev=True)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert float(a.float().abs().max()) >= 2.0 ** 13


# ------------------------------------------------------------------------------------------- 3. tsr_conv2d_fwd_f16s_pair
def test_pair_channel_perm_is_a_permutation(T):
    from tactilesr_amd._lib import call
    arr = (ctypes.c_int * 128)()
    call("tsr_pair_channel_perm", ctypes.cast(arr, ctypes.c_void_p))
    assert sorted(arr) == list(range(128))
    assert list(arr) == S.pair_perm().tolist()                 # the order the references of this file use
    from tactilesr_amd._lib import load
    assert load().tsr_pair_channel_perm(ctypes.c_void_p(0)) == 1


@pytest.mark.parametrize("case", S.PAIR_CASES, ids=S.cid)
def test_pair_one_launch(T, case):
    """conv3x3 || conv5x5 of one input slice as one launch, expected tensor in tsr_pair_channel_perm order."""
    one_launch("pair", case, S.pair_inputs, S.pair_ref, run_pair)


@pytest.mark.parametrize("case", S.PAIR_CASES, ids=S.cid)
def test_pair_3x3_half_equals_single_launch(T, case):
    """The 3x3 half of the pair launch against ONE tsr_conv2d_fwd_f16s 3x3 launch on the same input: 2 TOL (two fp32-grade
    evaluations of the same operation), per image."""
    p = S.pair_inputs(case)
    perm = S.pair_perm()
    got, _ = run_pair(p, case.offs)
    k3 = torch.nonzero(perm < 64).view(-1)                       # kernel channels of the 3x3 conv
    q = dict(x=p["x"], w=p["w3"], relu=p["relu"], res=None,
             scale=None if p["scale"] is None else p["scale"][k3][torch.argsort(perm[k3])],
             shift=None if p["shift"] is None else p["shift"][k3][torch.argsort(perm[k3])])
    single, _ = run_f16s(q, (case.offs[0], case.offs[1], 0))
    half = got[:, k3][:, torch.argsort(perm[k3])]                # logical channels 0..63 of the 3x3 conv
    per = S.check_images(half, single.double(), 2 * TOL)
    print(f"[pair vs single 3x3] {S.cid(case)}: {S.fmt_images(per)}")


# ------------------------------------------------------------------------------------------- 4. tsr_conv2d_fwd_f16s_fuse1x1
@pytest.mark.parametrize("case", S.FUSE_CASES, ids=S.cid)
def test_fuse1x1_one_launch(T, case):
    """act2(w2 . act(conv(x) * scale + shift) + shift2 + res): the stage-2 conv with its fused 64x128 1x1, res and out in
    different slices."""
    one_launch("fuse1x1", case, S.fuse_inputs, S.fuse_ref, run_fuse)


def test_fuse1x1_model_chain(T):
    """The two launches the model issues for MSRB stage 2 + `confusion`: P = W_a . stage3(x1) + b_c + x (3x3 launch, relu2 = 0),
    out = relu(W_b . stage5(x1) + P) (5x5 launch, res = P read from the slice the first launch wrote)."""
    from tactilesr_amd._lib import ptr
    B, H, W = 2, 13, 21
    g = torch.Generator().manual_seed(77)
    x1 = torch.randn(B, 128, H, W, generator=g) * 3
    x = torch.randn(B, 64, H, W, generator=g) * 3
    pa = dict(x=x1, w=S.he(g, 128, 128, 3), scale=torch.rand(128, generator=g) + 0.5, shift=torch.randn(128, generator=g) * 0.3,
              relu=1, w2=torch.randn(64, 128, 1, 1, generator=g) * (2.0 / 256) ** 0.5, shift2=torch.randn(64, generator=g) * 0.2,
              res=x, relu2=0)
    pb = dict(x=x1, w=S.he(g, 128, 128, 5), scale=torch.rand(128, generator=g) + 0.5, shift=torch.randn(128, generator=g) * 0.3,
              relu=1, w2=torch.randn(64, 128, 1, 1, generator=g) * (2.0 / 256) ** 0.5, shift2=None, res=None, relu2=1)
    refP = S.fuse_ref(pa)
    ref = S.fuse_ref(dict(pb, res=refP))
    assert S.image_ratio(refP) < 4 and S.image_ratio(ref) < 4
    a = fuse_args(pa, (16, 32, 48), prior=0.0)
    launch("tsr_conv2d_fwd_f16s_fuse1x1", FUSE_SIG, a)
    P, _ = S.read_slice(a["out"], B, 64, H, W, 32)
    perP = S.check_images(P, refP, TOL)
    assert a["out_amax"].item() == float(P.abs().max())
    b = fuse_args(pb, (48, 16, 0), prior=0.0)
    b.update(res=a["out"], res_ctot=64 + PAD, res_coff=32)       # P where the first launch left it
    launch("tsr_conv2d_fwd_f16s_fuse1x1", FUSE_SIG, b)
    out, _ = S.read_slice(b["out"], B, 64, H, W, 16)
    per = S.check_images(out, ref, TOL)
    print(f"[fuse1x1 chain] P {S.fmt_images(perP)}; out {S.fmt_images(per)}")
    assert b["out_amax"].item() == float(out.abs().max())


# ------------------------------------------------------------------------------------------- 5. the scale contract
def contract(kind, pow2=False):
    """(inputs, offsets, runner, reference) of the contract launch of `kind`; pow2: power-of-two scale, no shift / residual."""
    B, H, W = S.CONTRACT_B, S.CONTRACT_H, S.CONTRACT_W
    if kind == "k32_3x3":
        c = S.F16sCase(3, 64, 64, B, H, W, True, True, True, 1, "zero", (16, 32, 48))
        p, run, ref = S.f16s_inputs(c, 1), run_f16s, S.f16s_ref
    elif kind == "1x1":
        c = S.F16sCase(1, 128, 64, B, H, W, True, True, True, 1, "zero", (32, 48, 16))
        p, run, ref = S.f16s_inputs(c, 1), run_f16s, S.f16s_ref
    elif kind == "pair":
        c = S.PairCase(64, B, H, W, True, True, 1, "zero", (48, 16))
        p, run, ref = S.pair_inputs(c, 1), run_pair, S.pair_ref
    else:
        c = S.FuseCase(3, 64, B, H, W, 1, True, True, True, True, 1, "zero", (16, 48, 32))
        p, run, ref = S.fuse_inputs(c, 1), run_fuse, S.fuse_ref
    if pow2:
        n = p["scale"].numel()
        p = dict(p, scale=torch.pow(2.0, (torch.arange(n) % 5 - 2).float()), shift=None)
        for k in ("res", "shift2"):
            if k in p:
                p[k] = None
    return p, c.offs, run, ref


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kind", S.CONTRACT_KINDS)
def test_contract_same_binade(T, kind):
    """The kernels take only the exponent of in_amax: max|x| and the largest float of its binade give bit-identical results."""
    p, offs, run, _ = contract(kind)
    mx = float(p["x"].abs().max())
    top = math.ldexp(2.0 - 2.0 ** -23, math.frexp(mx)[1] - 1)
    assert mx <= top < 2 * mx and math.frexp(top)[1] == math.frexp(mx)[1] and float(f32(top).item()) == top
    g0, a0 = run(p, offs, in_amax=mx, prior=0.0)
    g1, a1 = run(p, offs, in_amax=top, prior=0.0)
    assert same(g0, g1) and same(a0.cpu(), a1.cpu())


@pytest.mark.parametrize("kind", S.CONTRACT_KINDS)
def test_contract_power_of_two_homogeneity(T, kind):
    """x * 2^k with in_amax * 2^k gives exactly 2^k times the k = 0 output and out_amax, k in {-60, -20, +20, +60}."""
    p, offs, run, _ = contract(kind, pow2=True)
    mx = float(p["x"].abs().max())
    g0, a0 = run(p, offs, in_amax=mx, prior=0.0)
    assert torch.isfinite(g0).all() and a0.item() == float(g0.abs().max())
    for k in S.HOMOGENEITY_K:
        f = 2.0 ** k
        xk = p["x"] * f
        assert torch.equal(xk.double(), p["x"].double() * f)               # (exact: no fp32 under- or overflow in the input)
        gk, ak = run(dict(p, x=xk), offs, in_amax=mx * f, prior=0.0)
        want = g0 * f
        assert torch.equal(want.double(), g0.double() * f)
        bad = int((gk.view(torch.int32) != want.view(torch.int32)).sum())
        print(f"[homogeneity] {kind} k={k}: {bad} of {gk.numel()} elements differ, out_amax {ak.item():.6e} vs {a0.item() * f:.6e}")
        assert bad == 0 and ak.item() == a0.item() * f


@pytest.mark.parametrize("kind", S.CONTRACT_KINDS)
def test_contract_loose_bound(T, kind):
    """in_amax = 2^j max|x| is a legal upper bound that costs j bits of the activation planes: error < 2^j TOL per image."""
    p, offs, run, ref_fn = contract(kind)
    ref = ref_fn(p)
    assert S.image_ratio(ref) < 4
    mx = float(p["x"].abs().max())
    errs = []
    for j in (0, 1, 2):
        got, am = run(p, offs, in_amax=mx * 2.0 ** j, prior=0.0)
        errs.append(float(S.check_images(got, ref, 2.0 ** j * TOL).max()))
        assert am.item() == float(got.abs().max())
    print(f"[loose bound] {kind}: j = 0, 1, 2 -> {errs[0]:.2e}, {errs[1]:.2e}, {errs[2]:.2e}")


@pytest.mark.parametrize("kind", S.CONTRACT_KINDS)
def test_contract_zero_input(T, kind):
    """x = 0 with in_amax = 0: the plain and pair launches give exactly act(shift + res) in fp32, fuse1x1 the fp64 reference of
    the same operation on a zero input at TOL; out_amax == max|got|."""
    p, offs, run, ref_fn = contract(kind)
    p = dict(p, x=torch.zeros_like(p["x"]))
    got, am = run(p, offs, in_amax=0.0, prior=0.0)
    if kind == "fuse1x1":
        per = S.check_images(got, ref_fn(p), TOL)
        print(f"[zero input] fuse1x1: {S.fmt_images(per)}")
    else:
        want = p["shift"].view(1, -1, 1, 1).expand_as(got).clone()
        if p.get("res") is not None:
            want = want + p["res"]                                        # one fp32 addition, as the epilogue does
        want = torch.relu(want) if p["relu"] else want
        assert torch.equal(got, want)
    assert am.item() == float(got.abs().max())


# ------------------------------------------------------------------------------------------- 6. refusals
def check_refusals(name, sig, args, mutations, width, ref):
    """Every mutated argument list returns 1 and launches nothing; the unmodified one returns 0 and meets the bar."""
    preset = args["out_amax"].item()
    for m in mutations:
        st = raw(name, sig, dict(args, **m))
        assert st == 1, f"{name} with {m}: status {st}"
    torch.cuda.synchronize()
    assert torch.isnan(args["out"]).all(), "a refused call wrote the output"
    assert args["out_amax"].item() == preset, "a refused call wrote out_amax"
    launch(name, sig, args)
    got, _ = S.read_slice(args["out"], args["B"], width, args["H"], args["W"], args["out_coff"])
    S.check_images(got, ref, TOL)
    print(f"[refusals] {name}: {len(mutations)} argument lists refused")


def test_f16s_refusals(T):
    c = S.REFUSAL_CASES["f16s"]
    p = S.f16s_inputs(c)
    a = f16s_args(p, c.offs, prior=7.0)
    check_refusals("tsr_conv2d_fwd_f16s", F16S_SIG, a, S.launch_mutations("f16s"), 64, S.f16s_ref(p))


def test_pair_refusals(T):
    c = S.REFUSAL_CASES["pair"]
    p = S.pair_inputs(c)
    a = pair_args(p, c.offs, prior=7.0)
    check_refusals("tsr_conv2d_fwd_f16s_pair", PAIR_SIG, a, S.launch_mutations("pair"), 128, S.pair_ref(p))


def test_fuse1x1_refusals(T):
    c = S.REFUSAL_CASES["fuse1x1"]
    p = S.fuse_inputs(c)
    a = fuse_args(p, c.offs, prior=7.0)
    check_refusals("tsr_conv2d_fwd_f16s_fuse1x1", FUSE_SIG, a, S.launch_mutations("fuse1x1"), 64, S.fuse_ref(p))


def test_pack_refusals(T):
    """The four pack routines: a refused call leaves the sentinel-filled buffer as it was."""
    from tactilesr_amd._lib import load
    SENT = 0x7A7A
    g = torch.Generator().manual_seed(9)
    n = 0
    for cout, cin, ks in S.PACK_SHAPES:
        w = dev(S.he(g, cout, cin, ks))
        wa = w.abs().max().reshape(1)
        buf = torch.full((load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 2),), SENT, dtype=torch.int16, device="cuda")
        host = dict(w=w, w_packed=buf, cout=cout, cin=cin, ks=ks, wscale=S.host_wscale(w.cpu()))
        for m in S.pack_host_mutations(cin):
            assert raw("tsr_pack_conv_weight_f16s", PACK_SIG, dict(host, **m)) == 1, m
        devv = dict(w=w, w_packed=buf, cout=cout, cin=cin, ks=ks, w_amax=wa)
        for m in S.pack_dev_mutations(cin):
            assert raw("tsr_pack_conv_weight_f16s_dev", PACK_DEV_SIG, dict(devv, **m)) == 1, m
        n += len(S.pack_host_mutations(cin)) + len(S.pack_dev_mutations(cin))
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), "a refused pack wrote its buffer"
        assert raw("tsr_pack_conv_weight_f16s", PACK_SIG, host) == 0
        torch.cuda.synchronize()
        assert not bool((buf == SENT).all())
    cin = S.PACK_PAIR_CIN
    w3, w5 = dev(S.he(g, 64, cin, 3)), dev(S.he(g, 64, cin, 5))
    wa = torch.maximum(w3.abs().max(), w5.abs().max()).reshape(1)
    buf = torch.full((load().tsr_conv_weight_pair_elems(cin),), SENT, dtype=torch.int16, device="cuda")
    pair = dict(w3=w3, w5=w5, w_packed=buf, cin=cin, wscale=S.host_wscale(w3.cpu(), w5.cpu()), w_amax=None)
    muts = S.pack_pair_mutations(cin)
    for m in muts:
        assert raw("tsr_pack_conv_weight_pair_f16s", PACK_PAIR_SIG, dict(pair, **m)) == 1, m
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), "a refused pack wrote its buffer"
    assert raw("tsr_pack_conv_weight_pair_f16s", PACK_PAIR_SIG, dict(pair, wscale=0.0, w_amax=wa)) == 0   # w_amax replaces wscale
    torch.cuda.synchronize()
    assert not bool((buf == SENT).all())
    print(f"[refusals] pack routines: {n + len(muts)} argument lists refused")
