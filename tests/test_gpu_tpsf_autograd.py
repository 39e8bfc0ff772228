"""tpsf_backward_ex (csrc/tpsf_mfma.hip) kernel by kernel, and the autograd of tactilesr_amd.tPSFNet through all four outputs to the
MLP, the taxels and the depth.

Yardstick and rule: tests/_tpsf_cases.py -- |kernel - fp64| <= max(1e-5 * scale, 4 * |fp32 oracle - fp64|) per element, the
scale being the quantity's own: a sample's max |d_depth|; a sample's largest gradient component, or the component itself for
the conditioned case under non-negative upstream gradients.  Upstream tables, scenarios and the fp32 rows:
tests/_tpsf_autograd.py (preconditions: tests/test_tpsf_autograd_cpu.py).  Exact expectations (== 0, torch.equal) are exact.
Every output is NaN-prefilled and carries a NaN guard band of one more sample, which must still be NaN afterwards; every
tpsf_backward_ex launch is issued twice into fresh buffers and must give the same bits.

  1. scenarios          dHR alone, dpsf alone, dLR_deg + dHR + dpsf, each with d_depth, on five case tables, two upstream kinds
  2. impulses           d_depth of a single-pixel dHR in closed form: exact zeros beyond +-49, seams, last wave, tile 3
  3. plateau            1e30 in dHR on the plateau changes no bit; all-plateau images; input pixels under the plateau
  4. compatibility      tpsf_backward_ex(dLR_deg only) == tpsf_backward bit for bit; d/dgamma always tpsf_backward's
  5. persistent walks   2100 different samples, every grid walks
  6. isolation          NaN / Inf in dHR, dpsf or depth of 16 samples leave the other 584 bit-identical
  7. module             tPSFNet: every parameter, x and depth against fp64 autograd; HR-only, psf-only, depth-only losses
"""
import functools
from collections import namedtuple

import pytest
import torch

import _tpsf_cases as T
import _tpsf_autograd as A

pytestmark = pytest.mark.gpu
NAN = float("nan")
Out = namedtuple("Out", "dab dd work")


def forward(depth, ab):
    """tpsf_forward: (depth, ab, HR) on the device."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    B = depth.shape[0]
    d, a_ = depth.contiguous().cuda(), ab.contiguous().cuda()
    HR = torch.empty(B, 100, 100, device="cuda")
    LR = torch.empty(B, 16, device="cuda")
    psf = torch.empty(B, 99, 99, device="cuda")
    call("tpsf_forward", ptr(d), ptr(a_), ptr(HR), ptr(LR), ptr(psf), I(B), stream())
    return d, a_, HR


def launch_ex_once(fwd, up, want_depth=True):
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    d, a_, HR = fwd
    B = d.shape[0]
    dev = [None if t is None else t.contiguous().cuda() for t in up]
    dab = torch.full((B + 1, 3), NAN, device="cuda")
    dd = torch.full((B + 1, 100, 100), NAN, device="cuda")
    work = torch.full((B + 1, 100, 100), NAN, device="cuda")
    call("tpsf_backward_ex", ptr(d), ptr(a_), ptr(HR), ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dab),
         ptr(dd) if want_depth else ptr(None), ptr(work), I(B), stream())
    torch.cuda.synchronize()
    out = [t.cpu() for t in (dab, dd, work)]
    for t in out:
        assert bool(torch.isnan(t[B:]).all())               # the guard band
    if not want_depth:
        assert bool(torch.isnan(out[1]).all())
    return Out(*(t[:B] for t in out))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def launch_ex(fwd, up, want_depth=True):
    """Two launches into fresh NaN-prefilled buffers: the same bits (work included, where it is written)."""
    o1, o2 = launch_ex_once(fwd, up, want_depth), launch_ex_once(fwd, up, want_depth)
    for q in Out._fields:
        assert same_bits(getattr(o1, q), getattr(o2, q)), q
    return o1


def launch_plain(fwd, dl):
    """tpsf_backward: (dab, work)."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    d, a_, HR = fwd
    B = d.shape[0]
    dab = torch.full((B + 1, 3), NAN, device="cuda")
    work = torch.full((B + 1, 100, 100), NAN, device="cuda")
    call("tpsf_backward", ptr(d), ptr(a_), ptr(HR), ptr(dl.contiguous().cuda()), ptr(dab), ptr(work), I(B), stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dab[B:]).all()) and bool(torch.isnan(work[B:]).all())
    return dab[:B].cpu(), work[:B].cpu()


@functools.lru_cache(maxsize=None)
def case_forward(name):
    case = T.CASES[name]()
    return case, forward(case.depth, case.ab)


# ------------------------------------------------------------------------------------------------------------- 1. scenarios
@pytest.mark.parametrize("name", A.AG_CASES)
def test_each_upstream_alone_and_all_together_with_the_depth_gradient(name):
    """For non-negative and for signed upstream gradients: dHR alone (dLR_deg NULL), dpsf alone, dLR_deg + dHR + dpsf, each with
    d_depth requested.  d(alpha, beta, gamma) per component / per sample and d_depth per sample against fp64 under the rule.
    Without dLR_deg d/dgamma is an exact 0; with dpsf alone d_depth is exactly 0 and `work` is not written."""
    case, fwd = case_forward(name)
    r32 = A.fp32_grads(name)
    rows = A.FP32_ROWS[name]
    for kind in A.KINDS:
        for mode in A.MODES:
            up = A.scenario_up(name, kind, mode)
            out = launch_ex(fwd, up)
            ref = A.grads64(case.depth, case.ab, up)
            g32 = r32[(kind, mode)]
            label = f"autograd {name} {kind} {mode}"
            T.check(f"{label} d(alpha, beta, gamma)", out.dab, ref.dab, A.dab_scale(name, kind, ref.dab), g32.dab, rows)
            T.check(f"{label} d_depth", out.dd, ref.dd, T.sample_scale(ref.dd), g32.dd, rows)
            if mode != "all":
                assert bool((out.dab[:, 2] == 0).all()), label
            if mode == "psf":
                assert bool((out.dd == 0).all()) and bool(torch.isnan(out.work).all()), label
            else:
                assert not bool(torch.isnan(out.work).any()), label
            if name != "degenerate":
                assert bool(torch.isfinite(out.dab).all()) and bool(torch.isfinite(out.dd).all()), label


# -------------------------------------------------------------------------------------------------------------- 2. impulses
def test_depth_gradient_of_single_pixel_dHR_in_closed_form():
    """dHR = one off-plateau pixel of value 1, 3e-3 or 2e4 at each of IMPULSE_ALL (corners, wave seams, rows 96..99, tile-3
    columns) under the wide PSF (band-edge tap 0.61) and two narrow ones: d_depth = alpha v g(y - y0) g(x - x0) to 1e-5 of its
    maximum, EXACTLY 0 beyond +-49 of the impulse.  Diagonal impulses give a bit-symmetric d_depth, as the forward's symmetry
    test holds for HR; an impulse and its transposed partner (different values v) are held to the rule against each other --
    the forward's test does not hold bit equality for those either."""
    depth, ab, dHR = A.impulse_inputs()
    fwd = forward(depth, ab)
    out = launch_ex(fwd, A.Up(None, dHR, None))
    B = len(T.IMPULSE_ALL)
    cf = torch.stack([A.impulse_dd_closed_form(i) for i in range(B)])
    T.check("autograd impulse d_depth vs closed form", out.dd, cf, T.sample_scale(cf))
    k = torch.arange(100)
    for i, (y0, x0) in enumerate(T.IMPULSE_ALL):
        far = ((k - y0).abs() > 49).view(-1, 1) | ((k - x0).abs() > 49).view(1, -1)
        assert bool(far.any()) and bool((out.dd[i][far] == 0).all()), (i, y0, x0)
        assert int((out.work[i] != 0).sum()) == 1 and float(out.work[i, y0, x0]) == float(dHR[i, y0, x0]), i
        if y0 == x0:
            assert torch.equal(out.dd[i], out.dd[i].t()), (i, y0, x0)
    for i, j in A.transposed_pairs():
        vi, vj = float(dHR[i].max()), float(dHR[j].max())
        a, b = out.dd[i].double() / vi, out.dd[j].double().t() / vj
        assert bool(((a - b).abs() <= 2 * T.BAR * float(a.abs().max())).all()), (i, j)
    assert bool(torch.isfinite(out.dd).all()) and bool((out.dab[:, 2] == 0).all())


# --------------------------------------------------------------------------------------------------------------- 3. plateau
def test_plateau_of_the_output_carries_no_gradient_and_the_input_under_it_receives_one():
    """Degenerate depths, dLR_deg + dHR + dpsf.  dHR = 1e30 on the plateau pixels only against dHR = 0: every bit of
    d(alpha, beta, gamma), d_depth and work is the same.  All-plateau images (constant, zeros): d_depth exactly 0, d/dalpha and
    d/dbeta bit for bit those of the dpsf-alone launch.  Block plateaus and the three-level depth: the depth pixels under the
    plateau receive the non-zero gradient fp64 gives them."""
    case, dpsf, zero, big, P = A.plateau_inputs()
    _, fwd = case_forward("degenerate")
    o0 = launch_ex(fwd, A.Up(case.dl, zero, dpsf))
    o1 = launch_ex(fwd, A.Up(case.dl, big, dpsf))
    for q in Out._fields:
        assert same_bits(getattr(o0, q), getattr(o1, q)), q
    assert bool((o1.work[P] == 0).all()) and bool(torch.isfinite(o1.dd).all()) and bool(torch.isfinite(o1.dab).all())
    ref = A.grads64(case.depth, case.ab, A.Up(case.dl, zero, dpsf))
    T.check("autograd plateau d(alpha, beta, gamma)", o0.dab, ref.dab, ref.dab.abs().amax(dim=1, keepdim=True))
    T.check("autograd plateau d_depth", o0.dd, ref.dd, T.sample_scale(ref.dd))
    alone = launch_ex(fwd, A.Up(None, None, dpsf))
    name = {n: i for i, n in enumerate(T.DEGENERATE)}
    for n in ("constant", "zeros"):
        i = name[n]
        assert bool((o0.dd[i] == 0).all()) and bool((o0.work[i] == 0).all()), n
        assert same_bits(o0.dab[i, :2], alone.dab[i, :2]) and float(o0.dab[i, 2]) == 0.0, n
        assert bool((o0.dab[i, :2] != 0).all()), n
    for n in ("block_tile3", "block_lastwave", "levels"):
        i = name[n]
        assert bool((o0.dd[i][P[i]] != 0).all()) and bool((ref.dd[i][P[i]] != 0).all()), n


# --------------------------------------------------------------------------------------------------------- 4. compatibility
@pytest.mark.parametrize("name", ["signed", "degenerate"])
def test_ex_with_dLR_deg_alone_is_tpsf_backward_and_gamma_is_always_its_own(name):
    """tpsf_backward_ex(dLR_deg, NULL, NULL, d_depth = NULL) == tpsf_backward in d_alpha_beta and work, bit for bit; with dHR
    and dpsf added (and d_depth requested) d/dgamma keeps tpsf_backward's bits."""
    case, fwd = case_forward(name)
    dab0, work0 = launch_plain(fwd, case.dl)
    o = launch_ex(fwd, A.Up(case.dl, None, None), want_depth=False)
    assert same_bits(o.dab, dab0) and same_bits(o.work, work0)
    for kind in A.KINDS:
        full = launch_ex(fwd, A.scenario_up(name, kind, "all"))
        assert same_bits(full.dab[:, 2], dab0[:, 2]), kind
    dab1, work1 = launch_plain(fwd, case.dl)               # and tpsf_backward itself is what it was: deterministic
    assert same_bits(dab1, dab0) and same_bits(work1, work0)


def test_refused_ex_calls_return_1_and_leave_the_outputs_untouched():
    from tactilesr_amd._lib import load, ptr
    lib = load()
    B = T.REFUSAL_TPSF_B
    shapes = {"depth": (B, 100, 100), "ab": (B, 3), "HR": (B, 100, 100), "dl": (B, 16), "dHR": (B, 100, 100),
              "dpsf": (B, 99, 99), "dab": (B, 3), "dd": (B, 100, 100), "work": (B, 100, 100)}
    buf = {k: torch.full(s, NAN, device="cuda") for k, s in shapes.items()}
    for label, args in A.refusal_table_ex(lambda name: ptr(buf[name])):
        assert lib.tpsf_backward_ex(*args) == 1, label
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool(torch.isnan(t).all()), k


# ------------------------------------------------------------------------------------------------------ 5. persistent walks
def test_persistent_walks_of_every_kernel_at_2100_different_samples():
    """One batch of 2100 different samples (tests/_persistent_loops.py: above the 2048 cap of the pool and psf kernels and the
    256 x occupancy caps of the GEMM kernels, magnitudes changing by decades from one iteration of a workgroup to the next), all
    three upstream gradients, d_depth requested: d(alpha, beta, gamma) against the sample's largest component and d_depth
    against the sample's maximum, fp64 matrix form, every sample whose pixels keep their distance from the plateau threshold
    (2086 of 2100, CPU test)."""
    from _persistent_loops import tpsf_inputs, TPSF_B
    depth, ab, dl = tpsf_inputs()
    dHR, dpsf = A.walk_upstream(TPSF_B, A.WALK_SEED)
    up = A.Up(dl, dHR, dpsf)
    out = launch_ex_once(forward(depth, ab), up)
    rows = A.walk_rows(depth)
    ref = A.grads64(depth, ab, up, rows)
    T.check("autograd walks d(alpha, beta, gamma)", out.dab[rows], ref.dab, ref.dab.abs().amax(dim=1, keepdim=True))
    T.check("autograd walks d_depth", out.dd[rows], ref.dd, T.sample_scale(ref.dd))
    assert bool(torch.isfinite(out.dab).all()) and bool(torch.isfinite(out.dd).all())


# ------------------------------------------------------------------------------------------------------------- 6. isolation
def test_nan_and_inf_in_dHR_dpsf_or_depth_stay_in_their_samples():
    """B = 600 (every grid but the pool / psf one walks; samples 256.., 512.. follow a poisoned sample in their workgroup): a
    NaN or Inf in dHR (samples 0..5), dpsf (6..10) or the depth (11..15, forward re-run) leaves d(alpha, beta, gamma) and
    d_depth of samples 16..599 bit-identical to the clean run."""
    n = T.ISOLATION_POISONED
    runs = []
    for poisoned in (False, True):
        depth, ab, dl, dHR, dpsf = A.isolation_inputs(poisoned)
        runs.append(launch_ex_once(forward(depth, ab), A.Up(dl, dHR, dpsf)))
    clean, dirty = runs
    assert bool(torch.isfinite(clean.dab).all()) and bool(torch.isfinite(clean.dd).all())
    assert same_bits(clean.dab[n:], dirty.dab[n:]) and same_bits(clean.dd[n:], dirty.dd[n:])
    assert not bool(torch.isfinite(dirty.dab[:n]).all(dim=1).any())               # the poison did reach its own samples


# ---------------------------------------------------------------------------------------------------------------- 7. module
MOD_BAR = 2e-5          # the bar tests/test_gpu_tpsf.py holds the MLP gradients to: 1e-5 for the PSF kernels, and as much again
#                         for the fp32 MLP (forward and backward GEMMs with fp32 accumulation) that (alpha, beta, gamma) and
#                         every gradient pass through; relative to the tensor's / the sample's largest entry


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


module_inputs = A.module_inputs


def module_net(psf=True, seed=7401):
    """tPSFNet with seeded parameters; psf: the returned psf is differentiable too (net.differentiable_psf, off by default)."""
    import tactilesr_amd
    from oracle import tactilesr_oracle as O
    sd = O.random_state_dict(O.tpsf_state_shapes(), seed)
    net = tactilesr_amd.tPSFNet(gama=1.4, perception_scale=None, device="cuda")
    net.load_state_dict(sd, strict=True)
    assert net.differentiable_psf is False
    net.differentiable_psf = psf
    return net.cuda(), sd


def module_loss(HR, LRd, psf, ab, w1, z, w2, w3, terms):
    B = HR.shape[0]
    loss = 0
    if "hr" in terms:
        loss = loss + (HR.reshape(B, 1, 100, 100) * w1).sum()
    if "lr" in terms:
        loss = loss + ((LRd.reshape(B, 1, 4, 4) - z) ** 2).mean()
    if "psf" in terms:
        loss = loss + (psf.reshape(B, 1, 99, 99) * w2).sum()
    if "ab" in terms:
        loss = loss + (ab.reshape(B, 1, 3) * w3).sum()
    return loss


@functools.lru_cache(maxsize=None)
def module_reference(terms):
    """fp64 autograd of O.tpsf_mlp + forward64: gradients of the eight MLP tensors, x and depth."""
    from oracle import tactilesr_oracle as O
    _, sd = module_net()
    x, depth, w1, z, w2, w3 = module_inputs()
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64, d64 = x.double().requires_grad_(True), depth.double().requires_grad_(True)
    ab = O.tpsf_mlp(p, x64)
    HR, LR, psf = T.forward64(ab, d64)
    loss = module_loss(HR, LR, psf, ab, w1.double(), z.double(), w2.double(), w3.double(), terms)
    gr = torch.autograd.grad(loss, list(p.values()) + [x64, d64], allow_unused=True)
    gr = [torch.zeros_like(t) if g is None else g for g, t in zip(gr, list(p.values()) + [x64, d64])]
    return dict(zip(list(p.keys()) + ["x", "depth"], gr))


def check_module(label, net, x, depth_leaf, ref, params=True):
    worst = 0.0
    if params:
        for k, p in net.named_parameters():
            e = relerr(p.grad, ref[k])
            worst = max(worst, e)
            assert e < MOD_BAR, (label, k, e)
    if x is not None:
        e = relerr(x.grad, ref["x"])
        worst = max(worst, e)
        assert x.grad.shape == x.shape and e < MOD_BAR, (label, "x", e)
    e = float(((depth_leaf.grad.detach().cpu().double().reshape(-1, 100, 100) - ref["depth"]).abs().flatten(1).amax(1)
               / ref["depth"].abs().flatten(1).amax(1).clamp_min(1e-300)).max())
    print(f"[tpsf autograd] module {label}: parameters / x worst {worst:.1e}, depth worst sample {e:.1e}")
    assert depth_leaf.grad.shape == depth_leaf.shape and e < MOD_BAR, (label, "depth", e)


@pytest.mark.parametrize("form", ["b1hw", "unsqueeze"])
def test_module_gradients_of_every_parameter_x_and_depth(form):
    """loss = sum HR w1 + mse(LR_deg, z) + sum psf w2 + sum alphaBeta w3: the eight MLP tensors, x (LR.requires_grad_()) and the
    depth, passed as a (B,1,100,100) leaf or through .unsqueeze(1) from a (B,100,100) leaf, against fp64 autograd."""
    net, _ = module_net()
    x, depth, w1, z, w2, w3 = module_inputs()
    xg = x.cuda().requires_grad_(True)
    if form == "b1hw":
        leaf = depth.unsqueeze(1).cuda().requires_grad_(True)
        arg = leaf
    else:
        leaf = depth.cuda().requires_grad_(True)
        arg = leaf.unsqueeze(1)
    HR, LRd, psf, ab = net(xg, arg)
    assert HR.requires_grad and psf.requires_grad and LRd.requires_grad and ab.requires_grad
    module_loss(HR, LRd, psf, ab, w1.cuda(), z.cuda(), w2.cuda(), w3.cuda(), ("hr", "lr", "psf", "ab")).backward()
    check_module(f"all terms, depth {form}", net, xg, leaf, module_reference(("hr", "lr", "psf", "ab")))


@pytest.mark.parametrize("terms", [("hr",), ("psf",)])
def test_module_loss_on_HR_alone_and_on_psf_alone(terms):
    """(HR * w).sum().backward() and the psf-only loss reach the MLP (and, for HR, the depth): both raise "does not require
    grad" without differentiable HR / psf outputs.  HR is differentiable as the module comes; psf once differentiable_psf is set
    (by default it stays the plain array existing callers read with .numpy())."""
    net, _ = module_net(psf=terms == ("psf",))
    x, depth, w1, z, w2, w3 = module_inputs()
    leaf = depth.unsqueeze(1).cuda().requires_grad_(True)
    HR, LRd, psf, ab = net(x.cuda(), leaf)
    assert HR.requires_grad and psf.requires_grad == (terms == ("psf",))
    module_loss(HR, LRd, psf, ab, w1.cuda(), z.cuda(), w2.cuda(), w3.cuda(), terms).backward()
    ref = module_reference(terms)
    check_module(f"{terms[0]} alone", net, None, leaf, ref)
    if terms == ("psf",):
        assert bool((leaf.grad == 0).all())
    else:
        assert bool((leaf.grad != 0).any())


def test_module_depth_gradient_alone_with_every_parameter_frozen():
    """The inverse problem: all parameters frozen, depth.requires_grad_() -- depth.grad is there and right, no parameter gets one."""
    net, _ = module_net()
    for p in net.parameters():
        p.requires_grad_(False)
    x, depth, w1, z, w2, w3 = module_inputs()
    leaf = depth.unsqueeze(1).cuda().requires_grad_(True)
    HR, LRd, psf, ab = net(x.cuda(), leaf)
    module_loss(HR, LRd, psf, ab, w1.cuda(), z.cuda(), w2.cuda(), w3.cuda(), ("hr", "lr")).backward()
    assert leaf.grad is not None and all(p.grad is None for p in net.parameters())
    check_module("depth alone, parameters frozen", net, None, leaf, module_reference(("hr", "lr")), params=False)


def test_trainer_loss_still_runs_tpsf_backward_bit_for_bit():
    """train_cal_loss (gradients through LR_deg only, no input gradient wanted) issues tpsf_backward, never tpsf_backward_ex,
    and its parameter gradients are bit for bit those of the parent commit's route: a direct tpsf_backward call on the module's
    own tensors with the dLR_deg autograd delivered, its result pushed through the MLP's backward chain."""
    import tactilesr_amd.model.tPSFNet as M
    from tactilesr_amd import functional as Fh
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    from tactilesr_amd.train import tPSFNet_train as TP
    net, _ = module_net(psf=False)
    x, depth, *_ = module_inputs()
    LR_raw, d = (x * 100).cuda(), depth.cuda()
    names, real = [], M.call
    M.call = lambda n, *a: (names.append(n), real(n, *a))[1]
    try:
        loss, _ = TP.train_cal_loss(net, (LR_raw, d), 100.0)
        loss.backward()
    finally:
        M.call = real
    assert "tpsf_backward" in names and "tpsf_backward_ex" not in names
    got = [p.grad.clone() for p in net.parameters()]

    def clear():
        for p in net.parameters():
            p.grad = None

    # the same loss by hand, to see the dLR_deg that autograd delivers
    clear()
    LR, d4 = LR_raw.float() / 100.0, d.float().unsqueeze(1)
    HR, LRd, psf, ab = net(LR, d4)
    seen = {}
    LRd.register_hook(lambda g: seen.__setitem__("dl", g.detach().clone()))
    Fh.mse_loss(LRd, LR[:, 2:3].contiguous()).backward()
    for p, g in zip(net.parameters(), got):
        assert torch.equal(p.grad, g)
    # the parent's route: tpsf_backward on the same tensors, then the MLP chain (entered through alphaBeta)
    B = LR.shape[0]
    dab = torch.full((B, 3), NAN, device="cuda")
    work = torch.empty(B * 10000, device="cuda")
    call("tpsf_backward", ptr(d.contiguous()), ptr(ab.detach().reshape(B, 3).contiguous()), ptr(HR.detach().contiguous()),
         ptr(seen["dl"].contiguous()), ptr(dab), ptr(work), I(B), stream())
    clear()
    ab2 = net(LR, d4)[3]
    ab2.backward(dab.view(B, 1, 3))
    for (k, p), g in zip(net.named_parameters(), got):
        assert torch.equal(p.grad, g), k
