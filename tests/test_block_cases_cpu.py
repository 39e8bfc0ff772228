"""The tables, data builders and fp64 references of tests/_block_cases.py, checked without a GPU: the case tables cover what
they claim, every data builder is well conditioned for the bars the device tests hold the kernels to, the hand-written
one-element-batch reference and the composed stack oracle agree with torch, and TrainFn refuses a second backward."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _block_cases as BC
from _gradcheck import check_pattern
from oracle import tactilesr_oracle as O

FLIP_TOL, MAX_FLIP_FRAC = check_pattern.__defaults__


def test_every_kind_and_arithmetic_is_in_both_tables():
    want = {(k, i) for k in BC.KINDS for i in BC.IMPLS}
    assert {c[:2] for c in BC.TRAIN_CASES} == want and {c[:2] for c in BC.EVAL_CASES} == want
    for k, i in want:          # ... at every size
        assert {c[2:] for c in BC.TRAIN_CASES if c[:2] == (k, i)} >= set(BC.SIZES)
        assert {c[2:] for c in BC.EVAL_CASES if c[:2] == (k, i)} == set(BC.SIZES)
    assert all(("res", i, 1, 1, 1) in BC.TRAIN_CASES for i in BC.IMPLS)
    assert len(set(BC.TRAIN_CASES)) == len(BC.TRAIN_CASES) and len(set(BC.EVAL_CASES)) == len(BC.EVAL_CASES)
    assert BC.AMP_SIZE in BC.SIZES and BC.PIXEL_SIZE in BC.SIZES and set(BC.AMP_K) == {-12, 0, 12}
    assert all(len(s) == 3 and set(s) <= set(BC.IMPLS) for s in BC.STACK_IMPLS)
    assert any(len(set(s)) == 3 for s in BC.STACK_IMPLS) and any(len(set(s)) == 1 for s in BC.STACK_IMPLS)


def _image_groups():
    """Images per workgroup of every conv launch a block engine issues, asked of the library: one 8x8 image gives one
    workgroup, whose slab entries are its image slots."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    return {lib.tsr_conv2d_slab_entries_ex(1, 8, 8, cout, ks, ns) for cout in (64, 128) for ks in (1, 3, 5)
            for ns in BC.NSPLIT.values()}


def test_sizes_hit_every_edge_of_the_tiling_and_of_the_image_groups():
    from tactilesr_amd import _lib
    lib = _lib.load()
    groups = {g for g in _image_groups() if g > 1}
    assert groups, "every launch form holds one image per workgroup?"
    S = BC.SIZES
    sub = [s for s in S if s[1] < 8 and s[2] < 8]
    assert len(sub) >= 2 and all(BC.tiles(h, w) == 1 for _, h, w in sub)                    # less than one tile
    assert any(h == 1 and w == 1 for _, h, w in sub) and any(h > 1 and w > 1 and h % 2 and w % 2 for _, h, w in sub)
    assert any(h == 8 and w == 8 and b % 2 == 1 and b > 1 for b, h, w in S)                 # exactly one tile, odd B
    assert any(h % 8 == 1 and h > 8 and w % 8 == 0 for _, h, w in S)                         # one row past a tile
    assert any(w % 8 == 1 and w > 8 and h % 8 == 0 for _, h, w in S)                         # one column past a tile
    assert any(h % 8 and w % 8 and h % 2 and w % 2 and BC.tiles(h, w) > 2 and all(b % g for g in groups) and b > max(groups)
               for b, h, w in S)                                                            # ragged, B a multiple of no group
    for g in groups:           # absent image slots in every grouping, a full workgroup in the smallest
        assert any(b % g for b, _, _ in S), g
    assert any(b % min(groups) == 0 for b, _, _ in S)
    assert (2, 40, 40) in S and all(h <= 40 and w <= 40 and b * h * w <= 2 * 40 * 40 for b, h, w in S)
    # the library's own entry count follows the formula the table was chosen by
    for b, h, w in S:
        for g in groups:
            ns, ks = next((ns, ks) for ns in BC.NSPLIT.values() for ks in (1, 3, 5)
                          if lib.tsr_conv2d_slab_entries_ex(1, 8, 8, 64, ks, ns) == g)
            assert lib.tsr_conv2d_slab_entries_ex(b, h, w, 64, ks, ns) == -(-b // g) * BC.tiles(h, w) * g


BUILDERS = ([(k,) + s + ({},) for k in BC.KINDS for s in BC.SIZES] + [("res", 1, 1, 1, {})]
            + [(k,) + BC.AMP_SIZE + ({"x_exp": e},) for k in BC.KINDS for e in BC.AMP_K if e]
            + [(k,) + BC.AMP_SIZE + ({"dy_exp": e},) for k in BC.KINDS for e in BC.AMP_K if e]
            + [(k,) + BC.AMP_SIZE + ({"x_zero": True},) for k in BC.KINDS]
            + [(k,) + BC.PIXEL_SIZE + ({"dy_mode": "pixel"},) for k in BC.KINDS])


@functools.lru_cache(maxsize=None)
def _sd(kind):
    return BC.make_block(kind)[1]


@pytest.mark.parametrize("kind,B,H,W,kw", BUILDERS, ids=[BC.case_id(b[:4]) + "".join(f"-{k}{v}" for k, v in b[4].items())
                                                          for b in BUILDERS])
def test_every_builder_is_well_conditioned_for_the_bars(kind, B, H, W, kw):
    """The oracle alone.  (1) A plain fp32 torch evaluation of the same graph stays under a quarter of every bar (TOL / 4 on
    the output, so on every pre-activation's scale).  (2) The pattern check cannot fail for a kernel that accurate: the
    pre-activations within TOL / 4 of zero -- all it can flip -- number at most max(4, max_flip_frac * total),
    check_pattern's own allowance, and each lies inside flip_tol.  (The share within the whole flip_tol is 2 * flip_tol *
    density(0) * max ~ 4e-5 for any bell-shaped pre-activation, twice max_flip_frac whatever the data: it is printed, not
    bounded.)  (3) No compared gradient tensor falls under the 1e-6 cut of check_grads (the dy-amplitude rows are compared
    after an exact rescaling by 2^-dy_exp), apart from the conv biases in front of a train-mode BatchNorm and, for x = 0,
    the gradients that vanish with x."""
    sd = _sd(kind)
    x, dy = BC.block_data(kind, B, H, W, **kw)
    r = BC.oracle_block(kind, sd, x, dy, record=True)
    total = sum(t.numel() for t in r.pre.values())
    near = round(BC.flip_fraction(r.pre, BC.TOL / 4) * total)
    print(f"[{kind} {B}x{H}x{W} {kw}] pre-activations within flip_tol of zero: {BC.flip_fraction(r.pre, FLIP_TOL):.1e} of "
          f"{total}; within TOL/4: {near}")
    assert BC.TOL / 4 < FLIP_TOL and near <= max(4, MAX_FLIP_FRAC * total), (near, total)
    scale = 2.0 ** -kw.get("dy_exp", 0)
    for k, g in r.grads.items():
        if BC.bias_before_train_bn(kind, k):
            assert float(g.abs().max()) * scale < 1e-6, k
        elif kw.get("x_zero") and float(g.abs().max()) < 1e-12:
            # the first convs' weight gradients (their input is 0) and, in the MSRB, the first stage's dgamma (zero batch
            # variance, xhat = 0); the second stage sees the zero padding at the border and is an ordinary BatchNorm
            assert k in ("conv1.weight", "conv_3_1.0.weight", "conv_5_1.0.weight", "conv_3_1.1.weight", "conv_5_1.1.weight"), k
        else:
            assert float(g.abs().max()) * scale >= 1e-6, (k, float(g.abs().max()))
    assert float(r.dx.abs().max()) * scale >= 1e-6
    worst = BC.conditioning(kind, sd, x, dy)
    assert worst < BC.TOL / 4, worst


def test_n2_builder_scales_x_into_the_linear_regime_of_batchnorm():
    """B*H*W = 2: with the unscaled law a plain fp32 evaluation already misses the bar (the BatchNorm backward is an
    O(eps/var) remainder), which is why the builder scales x there -- and only there."""
    sd = _sd("msrb")
    x, dy = BC.block_data("msrb", 2, 1, 1)
    unscaled, scaled = BC.conditioning("msrb", sd, x / BC.N2_X_SCALE, dy), BC.conditioning("msrb", sd, x, dy)
    print(f"[msrb 2x1x1] plain fp32 vs fp64: {unscaled:.2e} unscaled, {scaled:.2e} with x * 2^-12")
    assert unscaled > BC.TOL and scaled < BC.TOL / 4
    assert float(x.abs().max()) < 16 * BC.N2_X_SCALE
    x3, _ = BC.block_data("msrb", 1, 3, 5)
    assert float(x3.abs().max()) > 1 and float(BC.block_data("res", 2, 1, 1)[0].abs().max()) > 1


def test_bn_gain_reads_the_batch_variance_back():
    """Unit gain (a few) for the ordinary law, ~max|gamma| / sqrt(eps) where the batch variance vanishes."""
    sd = _sd("msrb")
    top = max(float(v.abs().max()) for k, v in sd.items() if k.endswith(".1.weight")) / O.BN_EPS ** 0.5
    for size, kw, lo, hi in (((3, 8, 8), {}, 1.0, 4.0), ((2, 40, 40), {}, 1.0, 4.0), ((3, 8, 8), {"x_zero": True}, 0.99 * top, top),
                             ((3, 8, 8), {"x_exp": -12}, 0.9 * top, top), ((2, 1, 1), {}, 0.9 * top, top)):
        x, dy = BC.block_data("msrb", *size, **kw)
        r = BC.oracle_block("msrb", sd, x, dy)
        assert lo <= BC.bn_gain(sd, r.ns, x.numel() // 64) <= hi * (1 + 1e-9), (size, kw)
    # the bar built on it: check_grads' own 1e-4 at unit gain, far above it where the variance vanishes
    x, dy = BC.block_data("msrb", 3, 8, 8)
    r = BC.oracle_block("msrb", sd, x, dy, record=True)
    assert set(r.gpre) == set(r.pre) and all(r.gpre[k].shape == r.pre[k].shape for k in r.pre)
    assert 1e-4 <= BC.zero_sum_bar(sd, r, 192) < 0.1
    x, dy = BC.block_data("msrb", 3, 8, 8, x_zero=True)
    assert BC.zero_sum_bar(sd, BC.oracle_block("msrb", sd, x, dy, record=True), 192) > 0.1
    # against the variance itself
    x, dy = BC.block_data("msrb", 3, 8, 8)
    z = F.conv2d(x.double(), sd["conv_3_1.0.weight"].double(), None, padding=1)
    g1 = float((sd["conv_3_1.1.weight"].double().abs() / torch.sqrt(z.var(dim=(0, 2, 3), unbiased=False) + O.BN_EPS)).max())
    ns = {k: v for k, v in BC.oracle_block("msrb", sd, x, dy).ns.items() if k.startswith("conv_3_1")}
    assert abs(BC.bn_gain(sd, ns, 192) - g1) < 1e-9 * g1


def test_msrb_one_element_batch_reference_vs_duplicated_batch():
    """torch refuses a one-value-per-channel train-mode BatchNorm; two IDENTICAL images have the same zero batch variance,
    the same xhat = 0 and (with dy duplicated) the same vanishing BatchNorm input gradients: the oracle on that batch gives
    the hand-written reference's output and dx per image, twice its parameter gradients, and its running statistics (the
    unbiased factor n/(n-1) multiplies a zero variance)."""
    sd = _sd("msrb")
    x, dy = BC.block_data("msrb", 1, 1, 1)
    with pytest.raises(ValueError, match="more than 1 value"):
        BC.oracle_block("msrb", sd, x, dy)
    ref = BC.msrb_n1_reference(sd, x, dy)
    dup = BC.oracle_block("msrb", sd, x.repeat(2, 1, 1, 1), dy.repeat(2, 1, 1, 1))
    for i in range(2):
        assert BC.relerr(dup.out[i:i + 1], ref.out) < 1e-12 and BC.relerr(dup.dx[i:i + 1], ref.dx) < 1e-12
    assert float(ref.out.abs().max()) > 0 and float(ref.dx.abs().max()) > 0
    for k, g in ref.grads.items():
        if float(g.abs().max()) == 0:
            assert float(dup.grads[k].abs().max()) < 1e-9, k
        else:
            assert BC.relerr(dup.grads[k], 2 * g) < 1e-12, k
    for k, v in ref.ns.items():
        assert BC.relerr(dup.ns[k], v) < 1e-12, k
        if k.endswith("running_var"):
            assert torch.equal(v, (1 - O.BN_MOMENTUM) * sd[k].double())


def _torch_stack_forward(mods, x):
    """Plain torch modules (the blocks' own nn.Sequential conv + BatchNorm + ReLU children), fp64, CPU."""
    def msrb(b, h):
        in2 = torch.cat([b.conv_3_1(h), b.conv_5_1(h)], 1)
        in3 = torch.cat([b.conv_3_2(in2), b.conv_5_2(in2)], 1)
        return F.relu(b.confusion(in3) + h)

    def res(b, h):
        return F.relu(h + b.conv2(F.relu(b.conv1(h))))
    return mods["cout"](res(mods["r"], msrb(mods["m1"], msrb(mods["m0"], mods["cin"](x)))))


def test_stack_oracle_vs_torch_autograd_through_module_copies():
    mods = BC.stack_modules()
    state = BC.stack_state(mods)
    x, target = BC.stack_data()
    loss, dx, grads, ns, out = BC.stack_oracle(state, x, target)
    for m in mods.values():
        m.double().train()
    xr = x.double().requires_grad_(True)
    out_t = _torch_stack_forward(mods, xr)
    loss_t = F.mse_loss(out_t, target.double())
    loss_t.backward()
    assert abs(loss - float(loss_t.detach())) < 1e-12 * abs(loss) and BC.relerr(out, out_t) < 1e-12 and BC.relerr(dx, xr.grad) < 1e-10
    named = {f"{n}.{k}": p for n, m in mods.items() for k, p in m.named_parameters()}
    assert set(named) == set(grads)
    gmax = max(float(g.abs().max()) for g in grads.values())
    for k, g in grads.items():
        assert float((g - named[k].grad).abs().max()) < 1e-10 * max(float(g.abs().max()), 1e-6 * gmax), k
    new = BC.stack_state(mods)
    assert ns and all(BC.relerr(new[k], v) < 1e-12 for k, v in ns.items() if not k.endswith("num_batches_tracked"))
    # on its own masks the forced oracle is the unforced one
    pre = {}
    tap = O.ReluTap(record=True)
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
    with torch.no_grad():
        BC.stack_forward64(p, x.double(), tap, True, {})
    loss_m, dx_m, grads_m, _, _ = BC.stack_oracle(state, x, target, masks={k: v > 0 for k, v in tap.pre.items()})
    assert loss_m == loss and torch.equal(dx_m, dx) and all(torch.equal(grads_m[k], grads[k]) for k in grads)
    # the gradient checks of the device test compare something: no tensor under the 1e-6 cut but the biases in front of BN
    for k, g in grads.items():
        blk = k.split(".", 1)
        if blk[0] in ("m0", "m1") and BC.bias_before_train_bn("msrb", blk[1]):
            assert float(g.abs().max()) < 1e-6, k
        else:
            assert float(g.abs().max()) >= 1e-6, (k, float(g.abs().max()))


class _ToyEngine:
    """What TrainFn needs of an engine, on the CPU: y = w * x."""

    def __init__(self, w):
        self.w, self.arena, self.backwards = w, None, 0

    def forward(self, x):
        class C:
            pass
        c = C()
        c.x = x.detach()
        return x.detach() * self.w.detach(), c

    def backward(self, c, dout):
        self.backwards += 1
        c.dx = dout * self.w.detach()
        return {"w": (dout * c.x).sum().reshape(1)}


def test_trainfn_refuses_a_second_backward_through_the_same_forward():
    """TrainFn.backward releases the forward's context; a second backward over a retained graph used to reach the engine
    with None and die there with an AttributeError."""
    from tactilesr_amd import _lib
    from tactilesr_amd.model._train import TrainFn
    w = torch.nn.Parameter(torch.tensor([3.0]))
    eng = _ToyEngine(w)
    x = torch.tensor([1.0, 2.0], requires_grad=True)
    loss = TrainFn.apply(eng, ["w"], x, w).sum()
    loss.backward(retain_graph=True)
    assert torch.equal(x.grad, torch.tensor([3.0, 3.0])) and torch.equal(w.grad, torch.tensor([3.0]))
    with pytest.raises(_lib.TactileSRHipError, match="second backward"):
        loss.backward()
    assert eng.backwards == 1
    # a fresh forward differentiates as before
    TrainFn.apply(eng, ["w"], x, w).sum().backward()
    assert eng.backwards == 2 and torch.equal(w.grad, torch.tensor([6.0]))
