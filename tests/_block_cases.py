"""Case tables, data builders and fp64 references of the standalone ``MSRB`` / ``ResBlock`` tests -- everything that runs
without a GPU (tests/test_block_cases_cpu.py checks the tables and the conditioning of every builder;
tests/test_gpu_block_cases.py and tests/test_gpu_blocks.py run the device side).

What is under test is how ``BlockEngine`` COMPOSES the train launches (the launches themselves have kernel-level tests):
NCHW <-> CB16 at the boundary, max|.| of the boundary tensors, the unmasked dx, the engine's own gradient arena -- in each
train arithmetic `block_engine()` accepts, at the sizes where the 8x8 tiling and the images-per-workgroup grouping have an edge.

SIZES (B, H, W) -- tiles = ceil(H/8) * ceil(W/8); a workgroup holds 2 or 4 images (tsr_conv2d_slab_entries_ex):
    (2, 1, 1)    less than one tile, the image smaller than every halo; B*H*W = 2 values per BatchNorm channel
    (1, 3, 5)    less than one tile, ragged on both axes, one image
    (3, 8, 8)    exactly one tile, odd B: absent image slots in both groupings
    (2, 9, 8)    one row past a tile
    (1, 8, 17)   one column past two tiles
    (5, 13, 21)  odd on both axes, B a multiple of no image group
    (2, 40, 40)  the workload's size, once
``("res", 1, 1, 1)`` is one more train row; ``("msrb", 1, 1, 1)`` is pinned against `msrb_n1_reference` (torch refuses it).

Data: `block_data` -- x = 2 * randn (signed: a block in a user network follows any layer), dy = randn, optionally scaled by a
power of two, zeroed, or reduced to one pixel of one image; `legacy=True` is the law the four old rows of
tests/test_gpu_blocks.py keep (post-ReLU-like x: half of it within 0.01 of zero, which piles the output ReLU's
pre-activations up at zero -- five times the near-zero share of the signed law, too many for a pattern check at 40x40).
At B*H*W = 2 a train-mode BatchNorm saturates: xhat = +-1/sqrt(1 + eps/var), and its backward is the O(eps/var) remainder of
three O(1) terms, so with var ~ 1 NO fp32 evaluation (torch's included) holds a 2e-5 bar on what lies below it.  The builder
therefore scales x of the MSRB's two-value case by `N2_X_SCALE` = 2^-12, which puts the first stage's var under eps and that
BatchNorm in its linear regime (measured: plain fp32 misses the bar unscaled and holds it by a factor of ten scaled);
`conditioning` measures, per builder, what a plain fp32 torch evaluation of the same graph makes of the bars.

References: `oracle_block` (train- or eval-mode BatchNorm, unforced or on given ReLU masks), `device_masks` (the masks of a
device context, under the oracle's names), `stack_forward64` / `stack_oracle` (conv -> MSRB -> MSRB -> ResBlock -> conv) and
`msrb_n1_reference` (the one-element batch, written out by hand).

Bars: TOL and GRAD_TOL, through tests/_gradcheck.check_pattern / check_grads.  One bar is restated: check_grads holds a
gradient whose exact value is 0 (the conv biases in front of a train-mode BatchNorm) to an ABSOLUTE 1e-4; where the batch
variance is far under eps (x = 0, x * 2^-12, two values per channel) BatchNorm backward multiplies by ~1/sqrt(eps) and that
absolute bar no longer describes rounding -- `zero_sum_bar` holds those cases to GRAD_TOL of the mass the sum cancels
(measured on an MI355X: 1.3e-01 against a cancelled mass of 3e+06, i.e. 4e-08 of it; 1e-4 absolute is kept everywhere else).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O

KINDS = ("msrb", "res")
IMPLS = ("fp16x3", "bf16x6", "f32")
NSPLIT = {"fp16x3": -2, "bf16x6": 3, "f32": 0}          # `nsplit` of the C ABI (include/tactilesr_hip.h)
TOL = 1e-5                                                # outputs, running statistics
GRAD_TOL = 2e-5                                           # dx and parameter gradients (tests/_gradcheck.check_grads)
SIZES = [(2, 1, 1), (1, 3, 5), (3, 8, 8), (2, 9, 8), (1, 8, 17), (5, 13, 21), (2, 40, 40)]
TRAIN_CASES = [(k, i) + s for k in KINDS for i in IMPLS for s in SIZES] + [("res", i, 1, 1, 1) for i in IMPLS]
EVAL_CASES = [(k, i) + s for k in KINDS for i in IMPLS for s in SIZES]
AMP_SIZE, AMP_K = (3, 8, 8), (-12, 0, 12)
PIXEL_SIZE = (5, 13, 21)
STACK_SIZE = (3, 13, 21)
STACK_IMPLS = [("fp16x3", "bf16x6", "f32"), ("f32", "fp16x3", "bf16x6"), ("fp16x3", "fp16x3", "fp16x3")]
STACK_BLOCKS = (("m0", "msrb"), ("m1", "msrb"), ("r", "res"))
N2_X_SCALE = 2.0 ** -12
SEED = 31


def case_id(c):
    return "-".join(str(v) for v in c)


def tiles(H, W):
    return ((H + 7) // 8) * ((W + 7) // 8)


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def randomise(block, seed):
    """Trained-like parameters: random BN affine / running statistics, biases (the seeded init has gamma = beta = 0.1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in block.state_dict().items():
            if k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.2)
            elif k.endswith(".1.weight"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    return {k: v.detach().clone() for k, v in block.state_dict().items()}


def make_block(kind, seed=SEED):
    """A seeded CPU module with trained-like parameters, and its state dict."""
    import tactilesr_amd
    torch.manual_seed(seed)
    blk = tactilesr_amd.MSRB() if kind == "msrb" else tactilesr_amd.ResBlock()
    return blk, randomise(blk, seed + 1)


def block_data(kind, B, H, W, seed=SEED, x_exp=0, dy_exp=0, x_zero=False, dy_mode="randn", legacy=False):
    """x, dy (fp32, CPU).  `x_exp` / `dy_exp`: scaled by that power of two; `dy_mode`: "randn", "zero", or "pixel" (non-zero
    at one pixel of one image, all channels)."""
    g = torch.Generator().manual_seed(seed + 2)
    if legacy:
        x = torch.randn(B, 64, H, W, generator=g).clamp_(min=0) * 2 + 0.01 * torch.randn(B, 64, H, W, generator=g)
    else:
        x = torch.randn(B, 64, H, W, generator=g) * 2
    dy = torch.randn(B, 64, H, W, generator=g)
    if kind == "msrb" and B * H * W == 2 and not legacy:
        x = x * N2_X_SCALE
    x = x * 2.0 ** x_exp
    if x_zero:
        x = torch.zeros_like(x)
    if dy_mode == "zero":
        dy = torch.zeros_like(dy)
    elif dy_mode == "pixel":
        keep = torch.zeros_like(dy)
        keep[B // 2, :, H // 2, W - 1] = 1
        dy = dy * keep
    return x, dy * 2.0 ** dy_exp


Ref = namedtuple("Ref", "out dx grads ns pre gpre", defaults=(None,))


class _GradTap(O.ReluTap):
    """ReluTap that also keeps the gradient arriving at every pre-activation (`gpre`: what enters BatchNorm backward)."""

    def __init__(self, masks=None, record=False):
        super().__init__(masks=masks, record=record)
        self.gpre = {}

    def __call__(self, name, x):
        if x.requires_grad:
            x.register_hook(lambda g, n=name: self.gpre.__setitem__(n, g.detach()))
        return super().__call__(name, x)


def _leaves(sd, prefix):
    p = {}
    for k, v in sd.items():
        v = v.detach().cpu()
        p[f"{prefix}.{k}"] = v.double().requires_grad_(O.is_trainable(k)) if v.is_floating_point() else v
    return p


def block_forward64(kind, p, prefix, x, training, ns, tap):
    if kind == "msrb":
        return O.msrb_forward(p, prefix, x, training=training, new_stats=ns, tap=tap)
    return O.resblock_forward(p, prefix, x, tap=tap)


def oracle_block(kind, sd, x, dy, masks=None, record=False, training=True, dtype=torch.float64):
    """One forward + backward of the CPU oracle: output, dx, {parameter: gradient}, new running statistics and (with
    `record`) the ReLU pre-activations; `masks` ("b.<name>" -> bool) forces the ReLU pattern; `training` = BatchNorm on batch
    statistics (False: the running ones, which stay).  Names carry no prefix on the way out, except `pre`'s "b."."""
    p = {k: (v.to(dtype).detach().requires_grad_(v.requires_grad) if v.is_floating_point() else v)
         for k, v in _leaves(sd, "b").items()}
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    tap = _GradTap(masks=masks, record=record) if (masks is not None or record) else None
    ns = {}
    ref = block_forward64(kind, p, "b", xr, training, ns, tap)
    names = [k for k, v in p.items() if v.is_floating_point() and v.requires_grad]
    gr = torch.autograd.grad((ref * dy.detach().cpu().to(dtype)).sum(), [xr] + [p[k] for k in names])
    return Ref(ref.detach(), gr[0], {k[2:]: g for k, g in zip(names, gr[1:])},
               {k[2:]: v.detach() for k, v in ns.items()}, tap.pre if tap is not None else None,
               tap.gpre if tap is not None else None)


def device_masks(kind, s, y, B, H, W, prefix="b"):
    """The ReLU pattern one block application took on the device, under the oracle's names: `s` is the block's saved
    context (`engine.last_ctx.s`), `y` its output.  BatchNorm pre-activations are re-evaluated in fp64 from the stored raw
    conv output and the scale / shift vectors the launches used."""
    from tactilesr_amd.model.tactileSR_model import from_cb16
    masks = {}

    def bn_mask(buf, ctot, coff, C, scale, shift):
        z = from_cb16(buf, B, C, H, W, ctot, coff).double().cpu()
        return (z * scale.double().cpu().view(1, -1, 1, 1) + shift.double().cpu().view(1, -1, 1, 1)) > 0

    if kind == "msrb":
        masks[f"{prefix}.conv_3_1.1"] = bn_mask(s.cat1, 128, 0, 64, s.bn_c1[0, :64], s.bn_c1[1, :64])
        masks[f"{prefix}.conv_5_1.1"] = bn_mask(s.cat1, 128, 64, 64, s.bn_c1[0, 64:], s.bn_c1[1, 64:])
        masks[f"{prefix}.conv_3_2.1"] = bn_mask(s.cat2, 256, 0, 128, s.bn_c2[0, :128], s.bn_c2[1, :128])
        masks[f"{prefix}.conv_5_2.1"] = bn_mask(s.cat2, 256, 128, 128, s.bn_c2[0, 128:], s.bn_c2[1, 128:])
    else:
        masks[f"{prefix}.conv1"] = from_cb16(s.F1.buf, B, 64, H, W).cpu() > 0
    masks[f"{prefix}.out"] = y.detach().cpu() > 0
    return masks


def flip_fraction(pre, flip_tol=1e-5):
    """Share of the recorded ReLU pre-activations within `flip_tol` (relative to their tensor's max) of zero: the elements
    at which `check_pattern` lets a right kernel disagree with fp64."""
    near = total = 0
    for t in pre.values():
        near += int((t.abs() < flip_tol * t.abs().max()).sum())
        total += t.numel()
    return near / max(total, 1)


def bias_before_train_bn(kind, name):
    """Conv biases in front of a train-mode BatchNorm: their exact gradient is zero."""
    return kind == "msrb" and name.endswith(".0.bias")


def bn_gain(sd, ns, n):
    """max over the train-mode BatchNorm layers and channels of |gamma| / sqrt(var + eps): the factor by which BatchNorm
    backward multiplies its incoming gradient (dz = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat))).  The batch
    variance is read back from the oracle's new running_var = (1 - m) * rv + m * var * n / (n - 1).
    Why the tests need it: the conv biases in front of a train-mode BatchNorm have the exact gradient sum(dz) = 0, and
    check_grads holds what the device makes of that sum to an ABSOLUTE 1e-4, which suits unit gain.  Where the batch
    variance is far under eps (x = 0, x * 2^-12, one or two values per channel) the gain is ~1/sqrt(eps) = 316 and the
    rounding of that sum grows with it: `zero_sum_bar` is the bar of such a case (the one-element batch, whose incoming
    gradient the hand-written reference does not carry, takes 1e-4 * gain)."""
    m, gain = O.BN_MOMENTUM, 0.0
    for k, rv_new in ns.items():
        if k.endswith("running_var"):
            var = (rv_new.double() - (1 - m) * sd[k].double()) / m * (max(n - 1, 1) / n)
            gamma = sd[k[:-len("running_var")] + "weight"].double()
            gain = max(gain, float((gamma.abs() / torch.sqrt(var.clamp(min=0) + O.BN_EPS)).max()))
    return gain


def zero_sum_bar(sd, ref, n, tol=GRAD_TOL):
    """The bar on a conv-bias gradient in front of a train-mode BatchNorm where the batch variance is small.  Its exact value
    is the sum over (b, h, w) of dz = gain * (g - mean(g) - xhat * mean(g * xhat)) = 0, so there is no tensor max to be
    relative to; what the sum cancels is gain_c * sum|g_c|, g the gradient entering BatchNorm backward (`ref.gpre`, from an
    `oracle_block` run with masks) and gain_c = |gamma_c| / sqrt(var_c + eps).  Held to the SAME relative `tol` as every other
    gradient, against that mass: max over layers and channels of tol * gain_c * sum|g_c| -- and never under check_grads' own
    absolute 1e-4, which is what the formula gives at unit gain for the sizes it was set at."""
    m, bar = O.BN_MOMENTUM, 1e-4
    for k, rv_new in ref.ns.items():
        if k.endswith("running_var"):
            layer = k[:-len(".running_var")]
            var = (rv_new.double() - (1 - m) * sd[k].double()) / m * (max(n - 1, 1) / n)
            gain = sd[layer + ".weight"].double().abs() / torch.sqrt(var.clamp(min=0) + O.BN_EPS)
            mass = ref.gpre["b." + layer].abs().sum(dim=(0, 2, 3))
            bar = max(bar, tol * float((gain * mass).max()))
    return bar


def conditioning(kind, sd, x, dy, training=True):
    """What a plain fp32 torch evaluation of the oracle's graph (CPU, the fp64 run's ReLU pattern) makes of the bars: worst
    relative error of output, dx and every compared parameter gradient against fp64.  A data builder is fit for the bars only
    if this stays well below them -- the HIP path is held to fp32-equivalent arithmetic, not to more.  The fp32 run leaves
    out the conv biases in front of a train-mode BatchNorm: they cancel exactly there, the train launches never add them
    (the bias only moves running_mean), and adding them in fp32 costs the digits of a small z."""
    r64 = oracle_block(kind, sd, x, dy, record=True, training=training)
    masks = {k: v > 0 for k, v in r64.pre.items()}
    sd32 = {k: (torch.zeros_like(v) if training and bias_before_train_bn(kind, k) else v) for k, v in sd.items()}
    r32 = oracle_block(kind, sd32, x, dy, masks=masks, training=training, dtype=torch.float32)
    worst = max(relerr(r32.out, r64.out), relerr(r32.dx, r64.dx))
    for k, g in r64.grads.items():
        if float(g.abs().max()) >= 1e-6:
            worst = max(worst, relerr(r32.grads[k], g))
    return worst


# ------------------------------------------------------------------------------------------------ the one-element batch
def msrb_n1_reference(sd, x, dy, momentum=O.BN_MOMENTUM):
    """MSRB in train mode on ONE value per channel (B = H = W = 1), by hand in fp64.  The batch variance is 0 and every xhat is
    0, so each BatchNorm outputs its beta: a1 = relu(beta1), a2 = relu(beta2), y = relu(Wc a2 + bc + x).  Backward: the
    BatchNorm input gradients vanish (g - mean(g) = 0 with one element), so dx = dy * [y > 0] (the residual path alone), the
    conv weights / biases and the gammas get 0, beta2 gets Wc^T dpre on a2's pattern, beta1 gets 0; running_mean moves towards
    the conv output (+ bias), running_var to (1 - m) * rv  (train_ops.hip: unbiased = n > 1 ? var * n / (n - 1) : var)."""
    d = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x, dy = x.double(), dy.double()
    b1 = torch.cat([d["conv_3_1.1.bias"], d["conv_5_1.1.bias"]])
    b2 = torch.cat([d["conv_3_2.1.bias"], d["conv_5_2.1.bias"]])
    a1, a2 = b1.clamp(min=0), b2.clamp(min=0)
    Wc = d["confusion.weight"].view(64, 256)
    pre = Wc @ a2 + d["confusion.bias"] + x.view(64)
    y = pre.clamp(min=0)
    dpre = dy.view(64) * (pre > 0)
    grads = {k: torch.zeros_like(v) for k, v in d.items() if O.is_trainable(k)}
    grads["confusion.weight"] = torch.outer(dpre, a2).view(64, 256, 1, 1)
    grads["confusion.bias"] = dpre
    db2 = (Wc.t() @ dpre) * (b2 > 0)
    grads["conv_3_2.1.bias"], grads["conv_5_2.1.bias"] = db2[:128], db2[128:]
    ns = {}
    centre = lambda w: w[:, :, w.shape[2] // 2, w.shape[3] // 2]       # a 1x1 image sees the centre tap alone
    for name, inp in (("conv_3_1", x.view(64)), ("conv_5_1", x.view(64)), ("conv_3_2", a1), ("conv_5_2", a1)):
        z = centre(d[f"{name}.0.weight"]) @ inp + d[f"{name}.0.bias"]
        ns[f"{name}.1.running_mean"] = (1 - momentum) * d[f"{name}.1.running_mean"] + momentum * z
        ns[f"{name}.1.running_var"] = (1 - momentum) * d[f"{name}.1.running_var"]
    return Ref(y.view(1, 64, 1, 1), dpre.view(1, 64, 1, 1), grads, ns, None)


# ------------------------------------------------------------------------------------- blocks stacked in a user network
def stack_modules(seed=SEED):
    """conv 3 -> 64, MSRB, MSRB, ResBlock, conv 64 -> 1 (CPU, fp32, seeded): {"cin", "m0", "m1", "r", "cout"}."""
    import tactilesr_amd
    torch.manual_seed(seed)
    mods = {"cin": torch.nn.Conv2d(3, 64, 3, padding=1), "m0": tactilesr_amd.MSRB(), "m1": tactilesr_amd.MSRB(),
            "r": tactilesr_amd.ResBlock(), "cout": torch.nn.Conv2d(64, 1, 3, padding=1)}
    for i, n in enumerate(("m0", "m1", "r")):
        randomise(mods[n], seed + 10 + i)
    return mods


def stack_state(mods):
    return {f"{n}.{k}": v.detach().cpu().clone() for n, m in mods.items() for k, v in m.state_dict().items()}


def stack_data(seed=SEED):
    B, H, W = STACK_SIZE
    g = torch.Generator().manual_seed(seed + 3)
    return torch.rand(B, 3, H, W, generator=g) * 4, torch.randn(B, 1, H, W, generator=g)


def stack_forward64(p, x, tap=None, training=True, ns=None):
    """The oracle composed from the same pieces (fp64): p is the prefixed state of `stack_state`."""
    h = F.conv2d(x, p["cin.weight"], p["cin.bias"], padding=1)
    for n, kind in STACK_BLOCKS:
        h = block_forward64(kind, p, n, h, training, ns, tap)
    return F.conv2d(h, p["cout.weight"], p["cout.bias"], padding=1)


def stack_oracle(state, x, target, masks=None, training=True):
    """loss = mse(out, target) of the fp64 stack, its gradient w.r.t. x and every parameter, the new running statistics,
    the output; on `masks` (prefixed "m0." / "m1." / "r.") when given."""
    p = {k: (v.detach().cpu().double().requires_grad_(O.is_trainable(k)) if v.is_floating_point() else v.cpu())
         for k, v in state.items()}
    xr = x.detach().cpu().double().requires_grad_(True)
    ns = {}
    out = stack_forward64(p, xr, O.ReluTap(masks=masks) if masks is not None else None, training, ns)
    loss = F.mse_loss(out, target.detach().cpu().double())
    names = [k for k, v in p.items() if v.is_floating_point() and v.requires_grad]
    gr = torch.autograd.grad(loss, [xr] + [p[k] for k in names])
    return float(loss.detach()), gr[0], dict(zip(names, gr[1:])), {k: v.detach() for k, v in ns.items()}, out.detach()


def adam_probe_check(w_dev, w_ref, w_start, g_ref, lr, weight_decay, name):
    """The bar of test_gpu_train.test_full_step_adam_vs_reference_golden on one tensor after the FIRST Adam step: that step
    moves every weight by lr * g' / (|g'| + eps), g' = g + wd * w -- by +-lr whatever |g'| is -- so a weight can differ from
    the reference's only where the SIGN of g' differs, i.e. where |g'| is below the gradient's noise floor.  Every element
    that differs must be such a near-zero-gradient one, must differ by at most 2 * lr (+5 %), and they must be few."""
    w_dev, w_ref = w_dev.detach().cpu().double(), w_ref.detach().cpu().double()
    diff = (w_dev - w_ref).abs()
    off = diff > 1e-6 + 1e-5 * w_ref.abs()
    gp = g_ref.double() + weight_decay * w_start.detach().cpu().double()
    assert float(diff.max()) <= 2.1 * lr and float(off.double().mean()) < 0.02, (name, float(diff.max()), float(off.double().mean()))
    if bool(off.any()):
        assert float(gp[off].abs().max()) < 3e-3 * float(gp.abs().max()), (name, float(gp[off].abs().max()), float(gp.abs().max()))
    return int(off.sum())
