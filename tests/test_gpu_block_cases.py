"""Standalone ``MSRB`` / ``ResBlock`` on the device against the fp64 oracle (tables, data and references: tests/_block_cases.py):
every train arithmetic `block_engine()` accepts and every eval arithmetic, at the sizes where the 8x8 tiling and the
images-per-workgroup grouping have an edge; amplitudes, zeros, held statistics, the one-element batch; blocks stacked between
torch layers with an engine and an arena each; and the autograd contract of ``TrainFn`` on a real engine (accumulation,
a shared MSRB, the refused second backward, a dropped graph).

Bars (the project's own, tests/test_gpu_blocks.py and tests/_gradcheck.py): output and running statistics 1e-5, dx and every
parameter gradient 2e-5 on the device's ReLU pattern, the pattern itself equal to fp64's up to rounding-zero flips.

Measured on an MI355X against the fp64 oracle, worst over the train table per (kind, arithmetic) -- every train case prints its
own figures and the running worst:
                      output (bar 1e-5)   dx (bar 2e-5)   parameter gradient (bar 2e-5)
    msrb  fp16x3          7.2e-07            7.1e-07            3.0e-06
    msrb  bf16x6          9.3e-07            7.5e-07            5.0e-06
    msrb  f32             8.6e-07            1.0e-06            2.6e-06
    res   fp16x3          1.6e-07            1.2e-07            6.6e-07
    res   bf16x6          1.8e-07            1.4e-07            6.2e-07
    res   f32             1.7e-07            1.2e-07            6.0e-07
Amplitude (x or dy times 2^-12 .. 2^12), x = 0, a one-pixel dy and held statistics stay inside the same range (worst parameter
gradient 4.7e-06, x = 0 under bf16x6); at most 1 ReLU flip per case.  fp16x3 holds the bars over the whole 2^-12 .. 2^12 range:
no range limit was met.  The eval forward: worst 1.3e-06.  The stack: loss 3.6e-08, input gradient 2.5e-06, parameter
gradients 2.8e-06; ~40 of 1.5 M weights differ after the first Adam step (sign of a gradient at its noise floor), the
second step's loss agrees to 1.9e-06.  Where the batch variance vanishes, a conv-bias gradient whose exact value is 0 reaches
1.3e-01 (x = 0, f32; the sum it is the rounding of cancels 3e+06) -- _block_cases.zero_sum_bar.
"""
import functools
import gc

import pytest
import torch
import torch.nn.functional as F

import _block_cases as BC
from _gradcheck import check_grads, check_pattern, oracle_grads, step_data
from oracle import tactilesr_oracle as O

pytestmark = pytest.mark.gpu
TOL, GRAD_TOL = BC.TOL, BC.GRAD_TOL
WORST = {}          # (kind, impl) -> [out, dx, parameter gradient]: the running worst over this session's train cases


@functools.lru_cache(maxsize=None)
def _sd(kind):
    return BC.make_block(kind)[1]


@functools.lru_cache(maxsize=None)
def _unforced(kind, B, H, W, kw, training=True):
    """The fp64 oracle on its own ReLU pattern (shared by the arithmetics of a case; never modified)."""
    x, dy = BC.block_data(kind, B, H, W, **dict(kw))
    return BC.oracle_block(kind, _sd(kind), x, dy, record=True, training=training)


def _module(kind, impl, sd, hold=False):
    import tactilesr_amd
    blk = tactilesr_amd.MSRB() if kind == "msrb" else tactilesr_amd.ResBlock()
    blk.load_state_dict(sd)
    blk.train_impl = blk.conv_impl = impl
    if hold:
        from tactilesr_amd.model.tactileSR_model import hold_bn_statistics
        hold_bn_statistics(blk)
    blk = blk.cuda().train()
    eng = blk.block_engine()
    eng.keep_ctx = True
    assert eng.impl == impl and eng.nsplit == BC.NSPLIT[impl] and eng.kind == kind
    return blk, eng


def _device_step(kind, impl, x, dy, hold=False):
    B, _, H, W = x.shape
    blk, eng = _module(kind, impl, _sd(kind), hold)
    xg = x.cuda().requires_grad_(True)
    y = blk(xg)
    y.backward(dy.cuda())
    masks = BC.device_masks(kind, eng.last_ctx.s, y, B, H, W)
    return blk, eng, y.detach(), xg.grad, masks


def _against_oracle(kind, blk, y, dx, masks, x, dy, unforced, training=True, grad_scale=1.0, small_var=False):
    """Output, running statistics, pattern, dx and every parameter gradient of one device step against the fp64 oracle on the
    device's masks.  `grad_scale` (a power of two, exact) brings both sides of a scaled-dy case back to unit amplitude in
    front of check_grads, whose zero cut is absolute; `small_var` marks a case whose batch variance lies far under eps: the
    exactly-zero bias gradients are then held to 2e-5 of the mass their sum cancels (_block_cases.zero_sum_bar), every other
    bar is as it was.  Returns (out, dx, worst parameter gradient) errors."""
    flips = check_pattern(masks, unforced.pre)
    r = BC.oracle_block(kind, _sd(kind), x, dy, masks=masks, training=training)
    e_out = BC.relerr(y, r.out)
    assert y.shape == r.out.shape and e_out < TOL, e_out
    new_sd = blk.state_dict()
    for k, v in r.ns.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert BC.relerr(new_sd[k], v) < TOL, k
        else:
            assert int(new_sd[k]) == int(v), k                         # num_batches_tracked advanced by one
    got = {k: p.grad * grad_scale for k, p in blk.named_parameters()}
    assert set(got) == set(r.grads) and all(bool(torch.isfinite(g).all()) for g in got.values())
    zero_tol = BC.zero_sum_bar(_sd(kind), r, x.numel() // 64) if small_var and training and kind == "msrb" else 1e-4
    if zero_tol > 1e-4:
        z = max(float(got[k].abs().max()) for k in got if BC.bias_before_train_bn(kind, k))
        print(f"[small batch variance] largest conv-bias gradient in front of BatchNorm {z:.2e}, bar {zero_tol:.2e}")
    worst = check_grads(got, {k: g * grad_scale for k, g in r.grads.items()}, tol=GRAD_TOL, zero_tol=zero_tol)
    e_dx = check_grads({"dx": dx * grad_scale}, {"dx": r.dx * grad_scale}, tol=GRAD_TOL)[0]
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(y).all())
    return e_out, e_dx, worst[0], flips


# ------------------------------------------------------------------------------------------------ train against fp64
@pytest.mark.parametrize("kind,impl,B,H,W", BC.TRAIN_CASES, ids=[BC.case_id(c) for c in BC.TRAIN_CASES])
def test_block_train_vs_fp64(kind, impl, B, H, W):
    """One train-mode forward + backward of a standalone block in `impl` against the fp64 oracle: output and running
    statistics within 1e-5, num_batches_tracked + 1, the ReLU pattern equal to fp64's up to rounding-zero flips, dx and every
    parameter gradient within 2e-5 on the device's pattern; then the no-grad train-mode call (forward only, statistics
    still moving).  (The MSRB's two-value row runs on x * 2^-12 and with the gain-scaled zero bar: _block_cases.py.)"""
    x, dy = BC.block_data(kind, B, H, W)
    blk, eng, y, dx, masks = _device_step(kind, impl, x, dy)
    unforced = _unforced(kind, B, H, W, ())
    e = _against_oracle(kind, blk, y, dx, masks, x, dy, unforced, small_var=kind == "msrb" and B * H * W == 2)
    w = WORST.setdefault((kind, impl), [0.0, 0.0, 0.0])
    w[:] = [max(a, b) for a, b in zip(w, e[:3])]
    print(f"[block train {kind} {impl} {B}x{H}x{W}] out {e[0]:.2e}, dx {e[1]:.2e}, worst param grad {e[2]:.2e}, {e[3]} flips; "
          f"worst so far of ({kind}, {impl}): out {w[0]:.2e}, dx {w[1]:.2e}, param grad {w[2]:.2e}")
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    with torch.no_grad():
        y2 = blk(x.cuda())
    assert BC.relerr(y2, unforced.out) < TOL and not y2.requires_grad
    if kind == "msrb":
        after = blk.state_dict()
        assert all(int(after[k]) == int(before[k]) + 1 for k in before if k.endswith("num_batches_tracked"))
        assert all(not torch.equal(after[k], before[k]) for k in before if k.endswith("running_mean"))


@pytest.mark.parametrize("impl", BC.IMPLS)
def test_msrb_train_on_a_one_element_batch(impl):
    """MSRB in train mode at (1, 1, 1): ONE value per BatchNorm channel.  torch raises here ("Expected more than 1 value per
    channel when training"); this library defines it (train_ops.hip: unbiased = n > 1 ? var * n / (n - 1) : var).  What the
    code does is pinned against the formula written out by hand in fp64 (_block_cases.msrb_n1_reference): zero batch
    variance, every BatchNorm outputs its beta, dx is the residual path alone, the conv weights and gammas get zero,
    running_var <- (1 - m) * running_var; everything finite."""
    kind = "msrb"
    x, dy = BC.block_data(kind, 1, 1, 1)
    sd = _sd(kind)
    ref = BC.msrb_n1_reference(sd, x, dy)
    blk, eng, y, dx, masks = _device_step(kind, impl, x, dy)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert BC.relerr(y, ref.out) < TOL
    got = {k: p.grad for k, p in blk.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    gain = max(float(v.abs().max()) for k, v in sd.items() if k.endswith(".1.weight")) / O.BN_EPS ** 0.5
    check_grads(got, ref.grads, tol=GRAD_TOL, zero_tol=1e-4 * gain)        # (zero batch variance: _block_cases.bn_gain)
    check_grads({"dx": dx}, {"dx": ref.dx}, tol=GRAD_TOL)
    zeros = max(float(got[k].abs().max()) for k, g in ref.grads.items() if float(g.abs().max()) == 0)
    print(f"[msrb one-element batch {impl}] largest entry of a gradient whose exact value is 0: {zeros:.2e} (bar {1e-4 * gain:.2e})")
    new_sd = blk.state_dict()
    for k, v in ref.ns.items():
        assert BC.relerr(new_sd[k], v) < TOL, k
        if k.endswith("running_var"):
            assert BC.relerr(new_sd[k], (1 - O.BN_MOMENTUM) * sd[k].double()) < 1e-6, k
    assert all(int(v) == 1 for k, v in new_sd.items() if k.endswith("num_batches_tracked"))


# ------------------------------------------------------------------------------------------------------- amplitude
AMP = [(k, i, w, e) for k in BC.KINDS for i in BC.IMPLS for w in ("x", "dy") for e in BC.AMP_K]


@pytest.mark.parametrize("kind,impl,which,k", AMP, ids=[f"{a}-{b}-{c}*2^{d}" for a, b, c, d in AMP])
def test_block_train_amplitude(kind, impl, which, k):
    """x (or, separately, dy) scaled by 2^k, k in {-12, 0, 12}, at (3, 8, 8): the same relative bars.  The fp16x3 operand
    scales come from max|x| and max|d| of the boundary tensors (BlockEngine.forward / backward), so a wrong scale shows here."""
    B, H, W = BC.AMP_SIZE
    kw = (("x_exp", k),) if which == "x" else (("dy_exp", k),)
    x, dy = BC.block_data(kind, B, H, W, **dict(kw))
    blk, eng, y, dx, masks = _device_step(kind, impl, x, dy)
    e = _against_oracle(kind, blk, y, dx, masks, x, dy, _unforced(kind, B, H, W, kw),
                        grad_scale=2.0 ** -k if which == "dy" else 1.0, small_var=which == "x" and k < 0)
    print(f"[block amplitude {kind} {impl} {which} * 2^{k}] out {e[0]:.2e}, dx {e[1]:.2e}, worst param grad {e[2]:.2e}")


# ----------------------------------------------------------------------------------------------------------- zeros
@pytest.mark.parametrize("impl", BC.IMPLS)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_block_train_zero_input(kind, impl):
    """x = 0 with a random dy: the operand amax of the boundary tensor is 0 and the MSRB's first-stage batch variance is 0;
    output and gradients finite and within the bars of the oracle."""
    B, H, W = BC.AMP_SIZE
    kw = (("x_zero", True),)
    x, dy = BC.block_data(kind, B, H, W, **dict(kw))
    assert float(x.abs().max()) == 0
    blk, eng, y, dx, masks = _device_step(kind, impl, x, dy)
    e = _against_oracle(kind, blk, y, dx, masks, x, dy, _unforced(kind, B, H, W, kw), small_var=True)
    print(f"[block x = 0 {kind} {impl}] out {e[0]:.2e}, dx {e[1]:.2e}, worst param grad {e[2]:.2e}")


@pytest.mark.parametrize("impl", BC.IMPLS)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_block_train_zero_cotangent(kind, impl):
    """dy = 0: dx and every parameter gradient exactly zero (and finite); the running statistics are those of a run with a
    random dy, bit for bit."""
    B, H, W = BC.AMP_SIZE
    x, dy = BC.block_data(kind, B, H, W)
    blk0, _, y0, dx0, _ = _device_step(kind, impl, x, torch.zeros_like(dy))
    blk1, _, y1, _, _ = _device_step(kind, impl, x, dy)
    assert torch.equal(y0, y1)
    assert bool(torch.isfinite(dx0).all()) and int(torch.count_nonzero(dx0)) == 0
    for n, p in blk0.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and int(torch.count_nonzero(p.grad)) == 0, n
    s0, s1 = blk0.state_dict(), blk1.state_dict()
    assert all(torch.equal(s0[k], s1[k]) for k in s0)


@pytest.mark.parametrize("impl", BC.IMPLS)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_block_train_single_pixel_cotangent(kind, impl):
    """dy non-zero at ONE pixel of ONE image of the (5, 13, 21) case (the last column, a ragged tile): the usual bars."""
    B, H, W = BC.PIXEL_SIZE
    kw = (("dy_mode", "pixel"),)
    x, dy = BC.block_data(kind, B, H, W, **dict(kw))
    assert int((dy.abs().sum(1) > 0).sum()) == 1
    blk, eng, y, dx, masks = _device_step(kind, impl, x, dy)
    e = _against_oracle(kind, blk, y, dx, masks, x, dy, _unforced(kind, B, H, W, kw))
    print(f"[block one-pixel dy {kind} {impl}] out {e[0]:.2e}, dx {e[1]:.2e}, worst param grad {e[2]:.2e}")


# ------------------------------------------------------------------------------------------------- eval against fp64
@pytest.mark.parametrize("kind,impl,B,H,W", BC.EVAL_CASES, ids=[BC.case_id(c) for c in BC.EVAL_CASES])
def test_block_eval_vs_fp64(kind, impl, B, H, W):
    """The eval forward in `conv_impl` against the oracle at 1e-5; then one train-mode forward, `.eval()` and a second
    forward, which must match the oracle's eval forward on the UPDATED running statistics (the packed plan is rebuilt)."""
    x, _ = BC.block_data(kind, B, H, W)
    sd = _sd(kind)
    blk, _ = _module(kind, impl, sd)
    blk.eval()

    def ref_of(state):
        p = {f"b.{k}": (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in state.items()}
        with torch.no_grad():
            return BC.block_forward64(kind, p, "b", x.double(), False, None, None)

    y = blk(x.cuda())
    ref = ref_of(sd)
    e0 = BC.relerr(y, ref)
    assert y.shape == ref.shape and not y.requires_grad and e0 < TOL, e0
    blk.train()
    with torch.no_grad():
        blk(x.cuda())
    blk.eval()
    new = blk.state_dict()
    y2 = blk(x.cuda())
    ref2 = ref_of(new)
    e1 = BC.relerr(y2, ref2)
    assert e1 < TOL, e1
    if kind == "msrb":
        assert all(not torch.equal(new[k].cpu(), sd[k]) for k in sd if k.endswith("running_var"))
        assert BC.relerr(ref2, ref) > 100 * TOL          # the statistics moved the answer: a stale plan would be seen
    else:
        assert torch.equal(y2, y)
    print(f"[block eval {kind} {impl} {B}x{H}x{W}] out {e0:.2e}, after a train-mode forward {e1:.2e}")


# ------------------------------------------------------------------------------------------------- held statistics
@pytest.mark.parametrize("impl", BC.IMPLS)
def test_msrb_train_with_held_statistics(impl):
    """hold_bn_statistics(MSRB()) in train mode at (2, 9, 8): output, dx and every gradient against the oracle with those
    layers in eval mode; running statistics and counters untouched bit for bit."""
    kind, (B, H, W) = "msrb", (2, 9, 8)
    x, dy = BC.block_data(kind, B, H, W)
    sd = _sd(kind)
    blk, eng, y, dx, masks = _device_step(kind, impl, x, dy, hold=True)
    assert blk.training and not blk.conv_3_1[1].training
    e = _against_oracle(kind, blk, y, dx, masks, x, dy, _unforced(kind, B, H, W, (), False), training=False)
    new = blk.state_dict()
    for k, v in sd.items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            assert torch.equal(new[k].cpu(), v), k
    print(f"[msrb held statistics {impl}] out {e[0]:.2e}, dx {e[1]:.2e}, worst param grad {e[2]:.2e}")


# -------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", BC.KINDS)
def test_block_refusals(kind):
    import tactilesr_amd
    from tactilesr_amd._lib import TactileSRHipError
    blk, _ = _module(kind, "fp16x3", _sd(kind))
    x = torch.zeros(1, 64, 3, 5)
    with pytest.raises(TactileSRHipError, match="no CPU fallback"):
        blk(x)
    with pytest.raises(AssertionError, match=r"take \(B, 64, H, W\) feature maps"):
        blk(torch.zeros(1, 32, 3, 5, device="cuda"))
    blk.train_impl = "bf16"
    with pytest.raises(TactileSRHipError, match=r"train_impl 'bf16' is not available \(fp16x3, bf16x6, f32\)"):
        blk(x.cuda())
    blk.train_impl = "fp16x3"
    blk.eval()
    blk.conv_impl = "bf16"
    with pytest.raises(TactileSRHipError, match=r"conv_impl 'bf16' is not available"):
        blk(x.cuda())
    blk.conv_impl = "fp16x3"
    assert blk(x.cuda()).shape == (1, 64, 3, 5)


# ------------------------------------------------------------------------------------- blocks stacked in a user network
def _stack_step(mods, engs, x, target):
    B, H, W = BC.STACK_SIZE
    xg = x.cuda().requires_grad_(True)
    h = mods["cin"](xg)
    ys = {}
    for n, _ in BC.STACK_BLOCKS:
        h = ys[n] = mods[n](h)
    out = mods["cout"](h)
    loss = F.mse_loss(out, target.cuda())
    loss.backward()
    masks = {}
    for n, kind in BC.STACK_BLOCKS:
        masks.update(BC.device_masks(kind, engs[n].last_ctx.s, ys[n], B, H, W, prefix=n))
    return float(loss.detach()), xg.grad, masks


@pytest.mark.parametrize("impls", BC.STACK_IMPLS, ids=["+".join(s) for s in BC.STACK_IMPLS])
def test_blocks_stacked_between_torch_layers(impls):
    """nn.Conv2d(3, 64) -> MSRB -> MSRB -> ResBlock -> nn.Conv2d(64, 1) at (3, 13, 21), the blocks in `impls` inside ONE autograd
    graph, each with its own engine, arena and dx handed to the layer in front.  Step 1 against the fp64 oracle composed from
    the same pieces on each block's own masks: loss 1e-5, the input gradient and every parameter gradient (torch layers and
    blocks) 2e-5, running statistics 1e-5.  Then tactilesr_amd.optim.Adam over all parameters against torch.optim.Adam on the
    fp64 oracle, at the bars of test_gpu_train.test_full_step_adam_vs_reference_golden: the weights after the first step
    (`adam_probe_check`), the second step's loss within 2e-4, no weight further than two steps' reach from the oracle's;
    after the second backward every block parameter's .grad aliases its own block's arena; last, an eval forward of the
    whole stack against the oracle's on the device's own parameters and statistics."""
    from tactilesr_amd import optim
    lr, wd = 1e-3, 1e-2
    mods = BC.stack_modules()
    state = BC.stack_state(mods)
    x, target = BC.stack_data()
    engs = {}
    for (n, _), impl in zip(BC.STACK_BLOCKS, impls):
        mods[n].train_impl = mods[n].conv_impl = impl
    for m in mods.values():
        m.cuda().train()
    for n, _ in BC.STACK_BLOCKS:
        engs[n] = mods[n].block_engine()
        engs[n].keep_ctx = True
    assert [engs[n].impl for n, _ in BC.STACK_BLOCKS] == list(impls)
    named = {f"{n}.{k}": p for n, m in mods.items() for k, p in m.named_parameters()}
    opt = optim.Adam(list(named.values()), lr=lr, weight_decay=wd)
    ref_p = {k: torch.nn.Parameter(state[k].double()) for k in named}
    ref_opt = torch.optim.Adam(list(ref_p.values()), lr=lr, weight_decay=wd)
    cur = dict(state)
    # ---- step 1
    loss, dx, masks = _stack_step(mods, engs, x, target)
    l64, dx64, g64, ns, _ = BC.stack_oracle(cur, x, target, masks)
    assert abs(loss - l64) < TOL * abs(l64), (loss, l64)
    worst = check_grads({k: p.grad for k, p in named.items()}, g64, tol=GRAD_TOL)
    e_dx = check_grads({"x": dx}, {"x": dx64}, tol=GRAD_TOL)[0]
    dev_state = BC.stack_state(mods)
    for k, v in ns.items():
        if not k.endswith("num_batches_tracked"):
            assert BC.relerr(dev_state[k], v) < TOL, k
    print(f"[stack {impls}] loss {abs(loss - l64) / abs(l64):.2e}, input gradient {e_dx:.2e}, worst parameter gradient "
          f"{worst[0]:.2e} ({worst[1]})")
    opt.step()
    for k in named:
        ref_p[k].grad = g64[k].clone()
    ref_opt.step()
    off = sum(BC.adam_probe_check(named[k], ref_p[k], state[k], g64[k], lr, wd, k) for k in named)
    cur.update(ns)
    cur.update({k: p.detach().clone() for k, p in ref_p.items()})
    # ---- step 2
    opt.zero_grad()
    assert all(p.grad is None for p in named.values())
    loss2, _, masks2 = _stack_step(mods, engs, x, target)
    l64b, _, g64b, _, _ = BC.stack_oracle(cur, x, target, masks2)
    assert abs(loss2 - l64b) <= 2e-4 * abs(l64b), (loss2, l64b)
    arenas = [engs[n].arena for n, _ in BC.STACK_BLOCKS]
    assert all(a is not None for a in arenas) and len({a.flat.data_ptr() for a in arenas}) == 3
    for n, _ in BC.STACK_BLOCKS:
        arena = engs[n].arena
        own = dict(mods[n].named_parameters())
        assert set(arena.names) == set(own)
        assert all(own[k].grad.data_ptr() == arena.flat.data_ptr() + 4 * arena.offsets[k] for k in arena.names), n
    opt.step()
    for k in named:
        ref_p[k].grad = g64b[k].clone()
    ref_opt.step()
    far = max(float((named[k].detach().cpu().double() - ref_p[k].detach()).abs().max()) for k in named)
    assert far <= 2 * 2.1 * lr, far
    assert int(opt.state[next(iter(named.values()))]["step"]) == 2
    print(f"[stack {impls}] {off} of {sum(p.numel() for p in named.values())} weights off after Adam step 1; second loss "
          f"{abs(loss2 - l64b) / abs(l64b):.2e}; farthest weight after step 2 {far:.2e}")
    # ---- eval forward on the device's own state
    for m in mods.values():
        m.eval()
    with torch.no_grad():
        h = mods["cin"](x.cuda())
        for n, _ in BC.STACK_BLOCKS:
            h = mods[n](h)
        out = mods["cout"](h)
        p = {k: (v.double() if v.is_floating_point() else v) for k, v in BC.stack_state(mods).items()}
        ref = BC.stack_forward64(p, x.double(), None, False, None)
    assert BC.relerr(out, ref) < TOL


# ------------------------------------------------------------------------ the autograd contract of TrainFn on a real engine
ACC_SIZE = (2, 9, 8)
NET_CFG = dict(scale_factor=3, patternFeatureExtraLayerCnt=1, forceFeatureExtraLayerCnt=1)


class _MsrbSubject:
    """One MSRB at (2, 9, 8): batches, a device step that ADDS into .grad, and the oracle gradient of a batch on its masks."""
    name = "msrb"

    def __init__(self):
        self.sd = _sd("msrb")
        self.m, self.eng = _module("msrb", "fp16x3", self.sd)
        B, H, W = ACC_SIZE
        self.batches = [BC.block_data("msrb", B, H, W, seed=BC.SEED + 7 * i) for i in range(2)]

    def forward_loss(self, i):
        x, dy = self.batches[i]
        return (self.m(x.cuda()) * dy.cuda()).sum()

    def backward(self, i):
        """device backward of batch i (accumulating); returns the oracle's gradient of that batch on the device's masks"""
        B, H, W = ACC_SIZE
        x, dy = self.batches[i]
        y = self.m(x.cuda())
        y.backward(dy.cuda())
        masks = BC.device_masks("msrb", self.eng.last_ctx.s, y, B, H, W)
        return BC.oracle_block("msrb", self.sd, x, dy, masks=masks).grads


class _NetSubject:
    """TactileSR(scale_factor=3, one MSRB, one ResBlock): the whole-network path through the same TrainFn."""
    name = "net"

    def __init__(self):
        import tactilesr_amd
        self.sd, _, _ = step_data(NET_CFG, 2, 51)
        self.batches = [step_data(NET_CFG, 2, 51 + 9 * i)[1:] for i in range(2)]
        m = tactilesr_amd.TactileSR(**NET_CFG)
        m.load_state_dict(self.sd, strict=True)
        self.m = m.cuda().train()
        self.eng = self.m.train_engine()
        self.eng.keep_ctx = True

    def forward_loss(self, i):
        LR, HR = self.batches[i]
        return F.mse_loss(self.m(LR.cuda()), HR.cuda())

    def backward(self, i):
        LR, HR = self.batches[i]
        self.forward_loss(i).backward()
        masks = {k: v.cpu() for k, v in self.eng.activation_masks(self.eng.last_ctx).items()}
        return oracle_grads(self.sd, LR, HR, scale_factor=NET_CFG["scale_factor"], masks=masks)[1]


SUBJECTS = {"msrb": _MsrbSubject, "net": _NetSubject}


def _grads(m):
    return {k: p.grad for k, p in m.named_parameters()}


def _aliases_arena(subject):
    arena, named = subject.eng.arena, dict(subject.m.named_parameters())
    return arena is not None and all(named[n].grad.data_ptr() == arena.flat.data_ptr() + 4 * arena.offsets[n] for n in arena.names)


@pytest.mark.parametrize("which", sorted(SUBJECTS))
def test_trainfn_gradient_accumulation(which):
    """backward(a), then backward(b) without zero_grad: .grad = g(a) + g(b) of the fp64 oracle (each batch on its own device
    masks; train-mode gradients do not depend on the running statistics the first step moved) within 2e-5, through the
    GradSink cases `first, accum` on a fresh module and `direct, accum` once the arena exists.  zero_grad(set_to_none=False)
    zeroes in place, so the next backward (still `accum`: the tensors are there) gives g(a) alone; after zero_grad() the next
    backward is `direct` again and .grad aliases the arena."""
    from test_gpu_frozen import _ModeLog
    s = SUBJECTS[which]()
    add = lambda a, b: {k: a[k] + b[k] for k in a}
    with _ModeLog() as log:
        ga = s.backward(0)
        gb = s.backward(1)
    assert log.modes == ["first", "accum"], log.modes
    w0 = check_grads(_grads(s.m), add(ga, gb), tol=GRAD_TOL)
    s.m.zero_grad(set_to_none=False)
    assert all(p.grad is not None and int(torch.count_nonzero(p.grad)) == 0 for p in s.m.parameters())
    with _ModeLog() as log:
        ga = s.backward(0)
    assert log.modes == ["accum"], log.modes
    w1 = check_grads(_grads(s.m), ga, tol=GRAD_TOL)
    s.m.zero_grad()
    with _ModeLog() as log:
        ga = s.backward(0)
        assert _aliases_arena(s)
        gb = s.backward(1)
    assert log.modes == ["direct", "accum"], log.modes
    w2 = check_grads(_grads(s.m), add(ga, gb), tol=GRAD_TOL)
    s.m.zero_grad()
    with _ModeLog() as log:
        gb = s.backward(1)
    assert log.modes == ["direct"] and _aliases_arena(s)
    w3 = check_grads(_grads(s.m), gb, tol=GRAD_TOL)
    print(f"[accumulation {which}] worst: first+accum {w0[0]:.2e}, zeroed in place {w1[0]:.2e}, direct+accum {w2[0]:.2e}, "
          f"direct {w3[0]:.2e}")


@pytest.mark.parametrize("which", sorted(SUBJECTS))
def test_trainfn_refuses_a_second_backward(which):
    """loss.backward(retain_graph=True), then loss.backward(): the first backward released the forward's context, so the
    second is refused by TrainFn with a message that names the cause -- not an AttributeError inside the engine -- and the
    module trains on as before."""
    from tactilesr_amd._lib import TactileSRHipError
    from test_gpu_frozen import _ModeLog
    s = SUBJECTS[which]()
    s.backward(0)                       # the arena exists
    s.m.zero_grad()
    loss = s.forward_loss(0)
    loss.backward(retain_graph=True)
    kept = {k: g.clone() for k, g in _grads(s.m).items()}
    with pytest.raises(TactileSRHipError, match="second backward through the same tactilesr_amd forward"):
        loss.backward()
    assert all(torch.equal(kept[k], g) for k, g in _grads(s.m).items())
    del loss
    s.m.zero_grad()
    with _ModeLog() as log:
        g = s.backward(0)
    assert log.modes == ["direct"] and _aliases_arena(s)
    check_grads(_grads(s.m), g, tol=GRAD_TOL)


@pytest.mark.parametrize("which", sorted(SUBJECTS))
def test_a_graph_dropped_without_backward_leaves_the_engine_unshared(which):
    """A forward that will never be differentiated (its graph is dropped), then a normal step: `direct`, aliasing the arena --
    the weak registration of note_forward does not leave the engine marked shared."""
    from test_gpu_frozen import _ModeLog
    s = SUBJECTS[which]()
    s.eng.keep_ctx = False              # (as a user runs it: nothing else holds the dropped forward's context)
    s.forward_loss(0).backward()        # the arena exists
    s.m.zero_grad()
    loss = s.forward_loss(1)
    assert loss.requires_grad and len(s.eng._live_forwards) == 1
    del loss
    gc.collect()
    assert len(s.eng._live_forwards) == 0
    s.eng.keep_ctx = True
    with _ModeLog() as log:
        g = s.backward(0)
    assert log.modes == ["direct"] and _aliases_arena(s) and not getattr(s.eng, "_shared_graph", False)
    check_grads(_grads(s.m), g, tol=GRAD_TOL)


@pytest.mark.parametrize("form", ["sum", "chain"])
def test_shared_msrb_applied_twice_in_one_graph(form):
    """ONE MSRB applied twice inside a single autograd graph -- `f(blk(a)) + f(blk(b))` and `blk(blk(x))` -- once its arena
    exists (test_gpu_blocks.test_shared_resblock_applied_twice_in_one_graph, with batch-statistics BatchNorm in each
    application): both backward passes take the `shared` case; outputs 1e-5, input gradients and every summed parameter
    gradient 2e-5 against the fp64 oracle with the shared parameters, each application on its own device masks; the step
    after it is a plain arena step again."""
    from test_gpu_frozen import _ModeLog
    B, H, W = ACC_SIZE
    sd = _sd("msrb")
    blk, eng = _module("msrb", "fp16x3", sd)
    (xa, da), (xb, db) = [BC.block_data("msrb", B, H, W, seed=BC.SEED + 7 * i) for i in range(2)]
    named = dict(blk.named_parameters())
    blk(xa.cuda()).backward(da.cuda())
    assert eng.arena is not None
    blk.zero_grad()
    a, b = xa.cuda().requires_grad_(True), xb.cuda().requires_grad_(True)
    y1 = blk(a)
    m1 = BC.device_masks("msrb", eng.last_ctx.s, y1, B, H, W)
    y2 = blk(b if form == "sum" else y1)
    m2 = BC.device_masks("msrb", eng.last_ctx.s, y2, B, H, W)
    loss = (y1 * da.cuda()).sum() + (y2 * db.cuda()).sum() if form == "sum" else (y2 * db.cuda()).sum()
    with _ModeLog() as log:
        loss.backward()
    assert log.modes == ["shared", "shared"], log.modes
    p64 = {f"b.{k}": (v.double().requires_grad_(O.is_trainable(k)) if v.is_floating_point() else v) for k, v in sd.items()}
    a64, b64 = xa.double().requires_grad_(True), xb.double().requires_grad_(True)
    r1 = O.msrb_forward(p64, "b", a64, training=True, new_stats={}, tap=O.ReluTap(masks=m1))
    r2 = O.msrb_forward(p64, "b", b64 if form == "sum" else r1, training=True, new_stats={}, tap=O.ReluTap(masks=m2))
    ref_loss = (r1 * da.double()).sum() + (r2 * db.double()).sum() if form == "sum" else (r2 * db.double()).sum()
    names = [k for k, v in p64.items() if v.is_floating_point() and v.requires_grad]
    ins = [a64, b64] if form == "sum" else [a64]
    grads = torch.autograd.grad(ref_loss, ins + [p64[k] for k in names])
    assert BC.relerr(y1, r1) < TOL and BC.relerr(y2, r2) < TOL
    got_in = {"a": a.grad, "b": b.grad} if form == "sum" else {"a": a.grad}
    check_grads(got_in, dict(zip(("a", "b"), grads[:len(ins)])), tol=GRAD_TOL)
    worst = check_grads({k: p.grad for k, p in named.items()}, {k[2:]: g for k, g in zip(names, grads[len(ins):])}, tol=GRAD_TOL)
    print(f"[shared msrb {form}] worst summed parameter gradient {worst[0]:.2e} ({worst[1]})")
    blk.zero_grad()
    with _ModeLog() as log:
        blk(xa.cuda()).backward(da.cuda())
    arena = eng.arena
    assert log.modes == ["direct"]
    assert all(named[n].grad.data_ptr() == arena.flat.data_ptr() + 4 * arena.offsets[n] for n in arena.names)
