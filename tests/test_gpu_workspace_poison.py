"""Every engine that chains launches, run on poisoned workspaces (tests/_poison.py).

Each case builds fresh, identically seeded objects and makes its call three times in one process: plainly, with every
`torch.empty` / `torch.empty_like` / `Tensor.new_empty` result filled with 0xFF bytes (NaN in every floating type) and filled
with 0x7B bytes (huge but finite: `fmaxf` and the max|x| atomics drop a NaN, a stale huge amax survives).  Every result --
outputs, the loss, every parameter gradient, LR.grad, BatchNorm buffers, optimizer and EMA state -- must be the plain run's
bit for bit, and the plain run finite and live.  There is no tolerance in this file: the plain run is held to the oracle by
the suites of the engines themselves; a difference here is a read of memory the call did not write.

Shapes: scale_factor 3 (12 x 12 = 2 x 2 ragged 8 x 8 tiles) at B = 1 and 3 (absent image slots in the 2- and 4-image
workgroups), one scale_factor 10, B = 2 case per engine; data from `_gradcheck.step_data` as in tests/_arch_cases.py.
"""
import functools

import pytest
import torch

import _block_cases as BC
import _frozen as FZ
import _gradcheck as GC
import _poison as P
from _engine_state import as_results, bits, cfg_of, ema_state, model_state, opt_state, tsr_model
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import optim
from tactilesr_amd.ema import WeightEMA
from tactilesr_amd.model.graph import GraphedForward
from tactilesr_amd.model.tactileSR_model import hold_bn_statistics
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

pytestmark = pytest.mark.gpu

SEED = 9500


# ------------------------------------------------------------------------------------------------------------ the harness
def check_runs(res, live=("out", "loss")):
    """`res`: {run label: {name: tensor}} with the label "plain" among them.  The plain run is finite and live, every other
    run has its names and its bits."""
    plain = res["plain"]
    assert plain, "the case returned nothing"
    for k, v in plain.items():
        if v.is_floating_point():
            assert bool(torch.isfinite(v).all()), f"plain run: {k} is not finite"
    for k, v in plain.items():
        if k.split(":")[0] in live:
            assert float(v.double().abs().max()) > 0, f"plain run: {k} is all zero"
    grads = [v for k, v in plain.items() if k.startswith("grad:")]
    if grads:
        assert sum(float(g.double().abs().max()) > 0 for g in grads) >= 0.9 * len(grads), "plain run: dead gradients"
    for label, got in res.items():
        if label == "plain":
            continue
        assert list(got) == list(plain), (label, sorted(set(got) ^ set(plain)))
        bad = []
        for k, v in plain.items():
            g = got[k]
            if g.shape != v.shape or g.dtype != v.dtype or not torch.equal(bits(g), bits(v)):
                nan = int(torch.isnan(g).sum()) if g.is_floating_point() else 0
                bad.append(f"{k} (NaN in {nan} of {g.numel()})")
        assert not bad, f"poison {label}: differs from the plain run in {len(bad)} of {len(plain)} results: {bad[:8]}"


def poison_check(case, live=("out", "loss"), plain_case=None):
    """Run `case()` plainly (or `plain_case()`, the eager twin of a graph case) and under both poisons; compare."""
    res = {}
    for label, ctx in P.runs():
        with ctx() as n:
            out = as_results((plain_case if label == "plain" and plain_case is not None else case)())
        torch.cuda.synchronize()
        assert label == "plain" or n[0] > 0, "the case allocated nothing through the patched names"
        res[label] = {k: v.cpu() for k, v in out.items()}
    check_runs(res, live)


def test_the_harness_sees_a_difference():
    """A case that reads its own unwritten workspace fails; one that does not passes."""
    x = torch.arange(1.0, 9.0, device="cuda")

    def clean():
        y = torch.empty_like(x)
        y.copy_(x * 2)
        return {"out": y}

    def dirty():
        y = torch.empty(8, device="cuda")
        y[:7] = x[:7]
        return {"out": y + 1}

    def stale_max():                       # a NaN is dropped by the maximum, the finite poison is not
        slot = torch.empty(1, device="cuda")
        return {"out": torch.fmax(slot, x.max().view(1))}
    poison_check(clean)

    def three(plain_result, fn):           # (what plain memory holds is not defined: the plain run is stated, not run)
        res = {"plain": {"out": plain_result.cpu()}}
        for label, ctx in P.runs()[1:]:
            with ctx():
                res[label] = {k: v.cpu() for k, v in as_results(fn()).items()}
        return res
    with pytest.raises(AssertionError, match="poison 0xFF: differs"):
        check_runs(three(x + 1, dirty))        # the workspace "happened to hold" last call's x
    res = three(x.max().view(1), stale_max)
    assert torch.equal(res["0xFF"]["out"], torch.tensor([8.0]))
    with pytest.raises(AssertionError, match="poison 0x7B: differs"):
        check_runs(res)


# ------------------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def tsr_data(T, M, R, sf, B):
    """(cfg, state dict, taxels, target) -- shared, never modified."""
    cfg = cfg_of(T, M, R, sf)
    return (cfg,) + GC.step_data(cfg, B, SEED + 100 * T + 10 * M + R + 1000 * sf + B)


# ------------------------------------------------------------------------------------------------------------ TactileSR eval
EVAL_VARIANTS = {
    "fp16x3": dict(conv_impl="fp16x3"),
    "fp16x3-two-stage1": dict(conv_impl="fp16x3", fuse_pair=False),
    "fp16x3-own-1x1": dict(conv_impl="fp16x3", fuse_1x1=False),
    "fp16x3-unfused": dict(conv_impl="fp16x3", fuse_pair=False, fuse_1x1=False),
    "bf16x6": dict(conv_impl="bf16x6"), "f32": dict(conv_impl="f32"), "bf16": dict(conv_impl="bf16"),
}
FULL_ARCHS = [(1, 2, 2), (3, 1, 1)]
COPY_ARCHS = [(1, 0, 1), (2, 1, 0), (1, 0, 0)]
EVAL_CASES = ([(a, v) for a in FULL_ARCHS for v in EVAL_VARIANTS] +
              [(a, v) for a in COPY_ARCHS for v in EVAL_VARIANTS if v != "bf16"])      # (bf16 storage needs M, R >= 1)


def eval_case(arch, variant, sf, B, **attrs):
    cfg, sd, LR, _ = tsr_data(*arch, sf, B)

    def case():
        m = tsr_model(cfg, sd, **EVAL_VARIANTS[variant], **attrs).eval()
        return {"out": m(LR.cuda())}
    return case


@pytest.mark.parametrize("arch,variant", EVAL_CASES, ids=[f"T{a[0]}M{a[1]}R{a[2]}-{v}" for a, v in EVAL_CASES])
def test_tactilesr_eval(arch, variant):
    for B in (1, 3):
        poison_check(eval_case(arch, variant, 3, B))


@pytest.mark.parametrize("variant", ["fp16x3", "bf16"])
def test_tactilesr_eval_scale_factor_10(variant):
    poison_check(eval_case((1, 2, 2), variant, 10, 2))


@pytest.mark.parametrize("variant", ["fp16x3", "fp16x3-unfused", "bf16x6", "f32", "bf16"])
def test_tactilesr_eval_in_passes_of_two(variant):
    """max_images_per_pass = 2 with B = 3: a pass of two images, then one of a single image on the blocks the first released."""
    poison_check(eval_case((1, 2, 2), variant, 3, 3, max_images_per_pass=2))


@pytest.mark.parametrize("arch,variant", [((1, 2, 2), "fp16x3"), ((3, 1, 1), "fp16x3-unfused"), ((1, 2, 2), "bf16"),
                                          ((1, 0, 0), "fp16x3"), ((2, 1, 0), "f32")],
                         ids=lambda v: v if isinstance(v, str) else "T%dM%dR%d" % v)
def test_forward_with_stages(arch, variant):
    cfg, sd, LR, _ = tsr_data(*arch, 3, 3)

    def case():
        m = tsr_model(cfg, sd, **EVAL_VARIANTS[variant]).eval()
        out, stages = m.forward_with_stages(LR.cuda())
        return {"out": out, **{"stage:" + k: v for k, v in stages.items()}}
    poison_check(case)


# ------------------------------------------------------------------------------------------------------------ TactileSR train
TRAIN_IMPLS = ("fp16x3", "bf16x6", "f32", "bf16", "bf16op")


def train_case(arch, impl, sf, B, prepare=None):
    cfg, sd, LR, HR = tsr_data(*arch, sf, B)

    def case():
        m = tsr_model(cfg, sd, train_impl=impl).train()
        if prepare is not None:
            prepare(m)
        x = LR.cuda().requires_grad_()
        out = m(x)
        loss = Fh.mse_loss(out, HR.cuda())
        loss.backward()
        return {"out": out, "loss": loss, "grad:LR": x.grad, **model_state(m)}
    return case


@pytest.mark.parametrize("impl", TRAIN_IMPLS)
@pytest.mark.parametrize("arch", FULL_ARCHS, ids=lambda a: "T%dM%dR%d" % a)
def test_tactilesr_train_step(arch, impl):
    for B in (1, 3):
        poison_check(train_case(arch, impl, 3, B))


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_tactilesr_train_step_scale_factor_10(impl):
    poison_check(train_case((1, 2, 2), impl, 10, 2))


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
@pytest.mark.parametrize("pattern", ["res_bias", "middle_msrb"])
def test_tactilesr_train_step_frozen_subset(pattern, impl):
    def freeze(m):
        named = dict(m.named_parameters())
        want, _ = FZ.PATTERNS[pattern](list(named))
        assert 0 < len(want) < len(named)
        for n, p in named.items():
            p.requires_grad_(n in want)
    poison_check(train_case((1, 2, 2), impl, 3, 3, prepare=freeze))


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_tactilesr_train_step_with_held_statistics(impl):
    def hold(m):
        hold_bn_statistics(m.patternFeatureExtra_layer[0])       # 4 BatchNorm layers of the first MSRB ...
        hold_bn_statistics(m.inputContact_layer)                 # ... and the fuse conv's
        hold_bn_statistics(m.patternFeatureExtra_layer[1].conv_3_1)      # a mixed stage-1 pair
        m.train()
    poison_check(train_case((1, 2, 2), impl, 3, 3, prepare=hold))


# ------------------------------------------------------------------------------------------------------------ standalone blocks
BLOCK_SIZES = [(3, 8, 8), (2, 9, 8)]


@functools.lru_cache(maxsize=None)
def block_inputs(kind, B, H, W):
    _, sd = BC.make_block(kind)
    return (sd,) + BC.block_data(kind, B, H, W)


def block_module(kind, sd):
    blk = tactilesr_amd.MSRB() if kind == "msrb" else tactilesr_amd.ResBlock()
    blk.load_state_dict(sd)
    return blk.cuda()


@pytest.mark.parametrize("impl", BC.IMPLS)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_standalone_block_eval(kind, impl):
    for size in BLOCK_SIZES:
        sd, x, _ = block_inputs(kind, *size)

        def case():
            blk = block_module(kind, sd).eval()
            blk.conv_impl = impl
            return {"out": blk(x.cuda())}
        poison_check(case)


@pytest.mark.parametrize("impl", BC.IMPLS)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_standalone_block_train(kind, impl):
    for size in BLOCK_SIZES:
        sd, x, dy = block_inputs(kind, *size)

        def case():
            blk = block_module(kind, sd).train()
            blk.train_impl = impl
            xin = x.cuda().requires_grad_()
            y = blk(xin)
            y.backward(dy.cuda())
            return {"out": y, "grad:x": xin.grad, **model_state(blk)}
        poison_check(case)


# ------------------------------------------------------------------------------------------------------------ TactileSRCNN
@functools.lru_cache(maxsize=None)
def srcnn_inputs():
    torch.manual_seed(SEED + 7)
    sd = BC.randomise(tactilesr_amd.TactileSRCNN(), SEED + 8)
    g = torch.Generator().manual_seed(SEED + 9)
    return sd, torch.rand(3, 3, 4, 4, generator=g) * 8


@pytest.mark.parametrize("impl", ["fp16x3", "bf16x6", "f32"])
def test_tactilesrcnn_eval(impl):
    sd, x = srcnn_inputs()

    def case():
        m = tactilesr_amd.TactileSRCNN()
        m.load_state_dict(sd)
        m = m.cuda().eval()
        m.conv_impl = impl
        return {"out": m(x.cuda())}
    poison_check(case)


# ------------------------------------------------------------------------------------------------------------ tPSFNet
@functools.lru_cache(maxsize=None)
def tpsf_inputs(B):
    torch.manual_seed(SEED + 20)
    sd = {k: v.clone() for k, v in tactilesr_amd.tPSFNet(0.5, 1.0).state_dict().items()}
    g = torch.Generator().manual_seed(SEED + 21 + B)
    x = torch.rand(B, 3, 4, 4, generator=g) * 8
    depth = torch.rand(B, 100, 100, generator=g) * 3
    depth[0, 40:60, 30:70] = 4.0                                   # a block plateau
    ups = (torch.randn(B, 1, 100, 100, generator=g) * 1e-4, torch.randn(B, 1, 4, 4, generator=g),
           torch.randn(B, 1, 99, 99, generator=g))
    return sd, x, depth, ups


def tpsf_net(sd):
    net = tactilesr_amd.tPSFNet(0.5, 1.0)
    net.load_state_dict(sd)
    return net.cuda()


@pytest.mark.parametrize("B", [3, 40])
def test_tpsfnet_trainer_loss(B):
    """MSE(LR[:, 2:3], LR_deg).backward(): the `tpsf_backward` path, two steps (the second reuses the slab of the first)."""
    sd, x, depth, _ = tpsf_inputs(B)

    def case():
        net = tpsf_net(sd)
        res = {}
        for step in range(2):
            net.zero_grad()
            HR, LRd, psf, ab = net(x.cuda(), depth.cuda())
            loss = torch.nn.functional.mse_loss(x.cuda()[:, 2:3], LRd)
            loss.backward()
            res.update({f"out:HR{step}": HR, f"out:LRd{step}": LRd, f"out:psf{step}": psf, f"out:ab{step}": ab,
                        f"loss:{step}": loss})
            res.update({f"{k}@{step}": v.clone() for k, v in model_state(net).items() if k.startswith("grad:")})
        return res
    poison_check(case)


@pytest.mark.parametrize("B", [3, 40])
def test_tpsfnet_full_autograd(B):
    """A loss on HR, LR_deg and psf with `differentiable_psf`, both inputs requiring grad: `tpsf_backward_ex`."""
    sd, x, depth, (uHR, uLR, upsf) = tpsf_inputs(B)

    def case():
        net = tpsf_net(sd)
        net.differentiable_psf = True
        xin, din = x.cuda().requires_grad_(), depth.cuda().requires_grad_()
        HR, LRd, psf, ab = net(xin, din)
        loss = (HR * uHR.cuda()).sum() + (LRd * uLR.cuda()).sum() + (psf * upsf.cuda()).sum() + ab.sum()
        loss.backward()
        return {"out:HR": HR, "out:LRd": LRd, "out:psf": psf, "out:ab": ab, "loss": loss, "grad:x": xin.grad,
                "grad:depth": din.grad, **model_state(net)}
    poison_check(case)


# ------------------------------------------------------------------------------------------------------------ functional
def images(B, H, W, seed, amp=25.0):
    g = torch.Generator().manual_seed(SEED + seed)
    return torch.rand(B, 1, H, W, generator=g) * amp, torch.rand(B, 1, H, W, generator=g) * amp


FN_SHAPES = [(3, 12, 12), (1, 12, 12), (2, 40, 40)]
KINDS = [("mse", None), ("l1", None), ("charbonnier", 1e-3), ("huber", 1.0)]
WEIGHTS = {1: (2.0,), 2: (0.0, 1.5), 3: (1.0, 0.0, 0.5)}


@pytest.mark.parametrize("B,H,W", FN_SHAPES)
def test_functional_losses(B, H, W):
    y, t = images(B, H, W, 30)
    g = torch.Generator().manual_seed(SEED + 31)
    z = torch.rand(B, 3, 4, 4, generator=g) * 8
    raw = torch.rand(B, 1, 100, 100, generator=g) * 250
    w = torch.tensor(WEIGHTS[B])
    gam = torch.rand(B, generator=g) + 0.3

    def case():
        Y, T_, Z, Wt = y.cuda(), t.cuda(), z.cuda(), w.cuda()
        res = {"out:prepare_target": Fh.prepare_target(raw.cuda(), 10.0, H // 4)}
        res["loss:mse"], res["out:mse_dy"] = Fh.mse_fwd_bwd(Y, T_)
        res["out:ssim11"] = Fh.ssim(Y, T_, 25.0, 11, 1.5)
        res["out:ssim3"] = Fh.ssim(Y, T_, 25.0, 3, 0.8)
        res["out:ssim_global"] = Fh.ssim(Y, T_, 25.0, 0)
        yg = Y.clone().requires_grad_()
        res["loss:ssim_loss"] = Fh.ssim_loss(yg, T_, 25.0)
        res["loss:ssim_loss"].backward()
        res["out:ssim_loss_dy"] = yg.grad
        s, stats = Fh.sample_scale(Wt, "sum")
        sb, statsb = Fh.sample_scale(Wt, "batch")
        res.update({"out:scale_sum": s, "out:scale_sum_stats": stats, "out:scale_batch": sb, "out:scale_batch_stats": statsb})
        for kind, param in KINDS:
            yg, tg = Y.clone().requires_grad_(), T_.clone().requires_grad_()
            loss = Fh.pixel_loss(yg, tg, kind, param, 4.0, 12.5)
            loss.backward()
            res.update({f"loss:pixel_{kind}": loss, f"out:pixel_{kind}_dy": yg.grad, f"out:pixel_{kind}_dt": tg.grad})
            pix, dy, dt = Fh.pixel_loss_per_sample(Y, T_, kind, param, 4.0, 12.5, scale=s, want_dt=True)
            res.update({f"out:ps_{kind}": pix, f"out:ps_{kind}_dy": dy, f"out:ps_{kind}_dt": dt})
        for name, gamma in (("scalar", 0.7), ("vector", gam.cuda())):
            q, lr_deg, dy, dz = Fh.degradation_fwd_bwd(Y, Z[:, 2], gamma, 10.0, want_dz=True)
            res.update({f"out:deg_{name}_q": q, f"out:deg_{name}_lr": lr_deg, f"out:deg_{name}_dy": dy, f"out:deg_{name}_dz": dz})
        res["out:deg_score"] = Fh.degradation_fwd_bwd(Y, Z[:, 2], 0.7, 10.0, want_dy=False)[0]
        res["out:degrade"] = Fh.degrade(Y, 0.7, 10.0)
        # every term on, without and with supervision weights
        parts = Fh.sr_loss_fwd_bwd(Y, T_, 0.1, 25.0, 11, 1.5, return_parts=True, pixel_kind="huber", pixel_param=1.0,
                                   fg_weight=4.0, fg_threshold=12.5, deg_weight=0.1, deg_z=Z[:, 2], deg_gamma=0.7, deg_gain=10.0)
        res.update({f"out:sr_{i}": v for i, v in enumerate(parts)})
        parts = Fh.sr_loss_fwd_bwd(Y, T_, 0.1, 25.0, 11, 1.5, return_parts=True, pixel_kind="huber", pixel_param=1.0,
                                   fg_weight=4.0, fg_threshold=12.5, deg_weight=0.1, deg_z=Z[:, 2], deg_gamma=gam.cuda(),
                                   deg_gain=10.0, sample_weight=Wt, sample_weight_norm="sum")
        res.update({f"out:srw_{i}": v for i, v in enumerate(parts)})
        ps, ss = Fh.psnr_ssim(Y, T_, 250.0)
        res.update({"out:psnr": ps, "out:ssim_quirk": ss, "out:wmean": Fh.weighted_mean(ps, s),
                    "out:mean": Fh.weighted_mean(ps)})
        return res
    # (a sample of scale 0 has an all-zero row in dy / dt: those results are live as a whole, which is what is asked)
    poison_check(case, live=("loss",))


def test_functional_data_paths():
    """dihedral (op list and index; planes and vector), taxel_noise, self_ensemble."""
    cfg, sd, LR, _ = tsr_data(1, 2, 2, 3, 3)
    g = torch.Generator().manual_seed(SEED + 40)
    x = torch.rand(5, 3, 4, 4, generator=g) * 8
    img = torch.rand(3, 1, 12, 12, generator=g)

    def case():
        X = x.cuda()
        res = {"out:dihedral": Fh.dihedral(X, ops=[0, 3, 5, 7, 2, 6, 1], index=[4, 0, 0, 2, 3, 1, 4]),
               "out:dihedral_vector": Fh.dihedral(X, ops=[7, 1, 4, 2, 6], axis_mode="vector"),
               "out:dihedral_all": Fh.dihedral(img.cuda(), op_all=5, scale=0.125),
               "out:dihedral_3d": Fh.dihedral(img.cuda()[:, 0], ops=[1, 2, 3])}
        acc = Fh.dihedral(img.cuda(), op_all=2, scale=0.5)
        res["out:dihedral_accumulate"] = Fh.dihedral(img.cuda(), op_all=4, out=acc, scale=0.5, accumulate=True)
        spec = dict(sigma_add=0.02, sigma_mul=(0.01, 0.02, 0.03), gain_jitter=0.05, drop_prob=0.1, drop_value=-1.0)
        res["out:taxel_noise"] = Fh.taxel_noise(X, spec, seed=3, offset=1, id_base=5)
        res["out:taxel_noise_ids"] = Fh.taxel_noise(X, spec, seed=3, ids=[9, 2, 2, 0, 7])
        res["out:taxel_noise_dev"] = Fh.taxel_noise(X, spec, rng=Fh.taxel_noise_rng(3, 4, "cuda"))
        for impl in ("fp16x3", "bf16"):
            m = tsr_model(cfg, sd, conv_impl=impl).eval()
            res["out:self_ensemble_" + impl] = Fh.self_ensemble(m, LR.cuda(), "dihedral")
            res["out:self_ensemble_vector_" + impl] = Fh.self_ensemble(m, LR.cuda(), (0, 1, 6), axis_mode="vector")
        return res
    poison_check(case)


# ------------------------------------------------------------------------------------------------------------ whole steps
def full_config(sf):
    return dict(TR.default_config(), scale_factor=sf, ssim_loss_weight=0.1, ssim_data_range=25.0, pixel_loss="huber",
                pixel_loss_param=1.0, contact_loss_weight=4.0, contact_threshold=12.5, degradation_loss_weight=0.1,
                degradation_gamma=0.7, sample_weight_norm="sum")


@functools.lru_cache(maxsize=None)
def step_batches(B, n, seed=50, amp_exp=()):
    """`n` 4-tuple batches (taxels rand * 8, raw targets rand * 250, gamma None, weights with a 0 where B > 1)."""
    g = torch.Generator().manual_seed(SEED + seed + B)
    out = []
    for i in range(n):
        s = 2.0 ** (amp_exp[i] if amp_exp else 0)
        w = torch.rand(B, generator=g) + 0.25
        if B > 1:
            w[(i + 1) % B] = 0.0
        out.append((torch.rand(B, 3, 4, 4, generator=g) * 8 * s, torch.rand(B, 1, 100, 100, generator=g) * 250 * s, None, w))
    return tuple(out)


def on_device(batch):
    return tuple(None if t is None else t.cuda() for t in batch)


# (lr 1e-5: Adam moves every weight by +-lr whatever its gradient, and at 1e-3 one step on these random weights pushes the
#  whole 40 x 40 output below the last ReLU -- the second step would compare all-zero gradients)
OPTIMS = {"adam": lambda ps: optim.Adam(ps, lr=1e-5, weight_decay=1e-2),
          "adamw-amsgrad": lambda ps: optim.AdamW(ps, lr=1e-5, weight_decay=1e-2, amsgrad=True)}


def trainer_objects(sf, B, opt_name, impl="fp16x3"):
    cfg, sd, _, _ = tsr_data(1, 2, 2, sf, B)
    m = tsr_model(cfg, sd, train_impl=impl).train()
    opt = OPTIMS[opt_name](m.parameters())
    ema = WeightEMA(m, decay=0.9, warmup=2, buffers="ema")
    return m, opt, ema


def step_results(parts_list, m, opt, ema):
    res = {}
    for i, parts in enumerate(parts_list):
        res.update({f"loss:{k}@{i}": v for k, v in parts.items()})
    return {**res, **model_state(m), **opt_state(opt, m), **ema_state(ema)}


@pytest.mark.parametrize("sf,B", [(3, 3), (3, 1), (10, 2)])
@pytest.mark.parametrize("opt_name", list(OPTIMS))
def test_train_one_iter_fullest_config(opt_name, sf, B):
    """SSIM + Huber with a contact weight + the degradation term + sample weights + clip_grad_norm + a WeightEMA, two steps
    (the second writes the gradient arena and the tables the first laid out)."""
    conf = full_config(sf)
    batches = step_batches(B, 2)

    def case():
        m, opt, ema = trainer_objects(sf, B, opt_name)
        parts = []
        for b in batches:
            p = TR.train_one_iter(m, opt, on_device(b), conf, clip_grad_norm=1.0, ema=ema)
            parts.append({k: v.detach().clone() for k, v in p.items()})
        return step_results(parts, m, opt, ema)
    poison_check(case)


@pytest.mark.parametrize("sf,B", [(3, 3), (10, 2)])
def test_eval_func_every_option(sf, B):
    conf = full_config(sf)
    batches = step_batches(B, 2, seed=60) + step_batches(1, 1, seed=61)      # a short last batch

    def case():
        m, opt, ema = trainer_objects(sf, B, "adam")
        TR.train_one_iter(m, opt, on_device(batches[0]), conf, ema=ema)      # the average differs from the weights
        scores = TR.eval_func(m, [on_device(b) for b in batches], conf, windowed_ssim=True, self_ensemble="dihedral",
                              ema=ema, taxel_noise=dict(sigma_add=0.02, gain_jitter=0.05, drop_prob=0.1), noise_seed=7,
                              degradation=True)
        assert len(scores) == 5
        return {"out:scores": torch.tensor(scores, dtype=torch.float64), **model_state(m), **ema_state(ema)}
    poison_check(case)


# ------------------------------------------------------------------------------------------------------------ graph classes
@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
@pytest.mark.parametrize("sf,B", [(3, 3), (10, 2)])
def test_graphed_train_step(sf, B, impl):
    """Construct, capture and replay three batches under poison (the fills are captured: every replay poisons again), against
    the eager plain run of the same four steps."""
    conf = full_config(sf)
    batches = step_batches(B, 4, seed=70)

    def steps(graphed):
        m, opt, ema = trainer_objects(sf, B, "adam", impl)
        step = GraphedTrainStep(m, opt, dict(conf), warmup=1, clip_grad_norm=1.0, ema=ema) if graphed else None
        parts = []
        for b in batches:
            p = step(on_device(b)) if graphed else TR.train_one_iter(m, opt, on_device(b), conf, clip_grad_norm=1.0, ema=ema)
            parts.append({k: v.detach().clone() for k, v in p.items()})
        assert not graphed or step.captures == 1
        return step_results(parts, m, opt, ema)
    poison_check(lambda: steps(True), plain_case=lambda: steps(False))


@pytest.mark.parametrize("variant", ["fp16x3", "fp16x3-unfused", "bf16"])
@pytest.mark.parametrize("arch,sf,B", [((1, 2, 2), 3, 3), ((1, 0, 0), 3, 3), ((1, 2, 2), 10, 2)],
                         ids=["T1M2R2-sf3-B3", "T1M0R0-sf3-B3", "T1M2R2-sf10-B2"])
def test_graphed_forward(arch, sf, B, variant):
    if variant == "bf16" and min(arch[1:]) == 0:
        variant = "bf16x6"                                          # (bf16 storage needs M, R >= 1: the copy path in bf16x6)
    cfg, sd, LR, _ = tsr_data(*arch, sf, B)
    g = torch.Generator().manual_seed(SEED + 80)
    xs = [LR] + [torch.rand(LR.shape, generator=g) * 8 for _ in range(2)]

    def run(graphed):
        m = tsr_model(cfg, sd, **EVAL_VARIANTS[variant]).eval()
        f = GraphedForward(m, xs[0].cuda()) if graphed else m
        return {f"out:{i}": f(x.cuda()).clone() for i, x in enumerate(xs)}
    poison_check(lambda: run(True), plain_case=lambda: run(False))
