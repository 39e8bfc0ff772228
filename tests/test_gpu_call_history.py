"""State that outlives a call: one object driven through a sequence of calls, each call's full result compared
(`torch.equal`, NaN nowhere) with a fresh object that was given the same state and made only that call.

What persists across calls and could go stale: plan caches keyed on (address, version) and the library's parameter epoch,
the tPSFNet gradient plan's split-K slab (`ns = min(32, ceil(B / 16))` changes with B), gradient arenas, the Adam / EMA chunk
tables, the static buffers and baked scales of the two graph classes, and the caching allocator's blocks, which hand a
smaller batch the memory a larger one just filled.  The amplitude ladder of the graph tests exists because the fp16x3 input
scale is 2^(13 - floor(log2 amax)): batches of one amplitude land in one bucket on every replay, and a max|x| slot or a scale
baked at capture would pass (`test_the_ladder_crosses_power_of_two_buckets`, no GPU, shows the ladder does not).
"""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import _block_cases as BC
import _gradcheck as GC
from _engine_state import cfg_of, ema_state, fresh_like, model_state, opt_state, same_results, tsr_model
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import optim
from tactilesr_amd.ema import WeightEMA, recalibrate_bn
from tactilesr_amd.model.graph import GraphedForward
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

gpu = pytest.mark.gpu

SEED = 9700
SF = 3
ARCH = (1, 2, 2)
CFG = cfg_of(*ARCH, SF)
LADDER = (0, 5, -5, 0)                      # taxels and targets scaled by 2^k


def batch(B, seed, exp=0, sf=SF):
    """Taxels rand * 8 and a target rand * 25 at 4 sf x 4 sf (`_gradcheck.step_data`'s law), both scaled by 2^exp."""
    g = torch.Generator().manual_seed(SEED + seed)
    s = 2.0 ** exp
    return torch.rand(B, 3, 4, 4, generator=g) * 8 * s, torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25 * s


def raw_batch(B, seed, exp=0):
    """The trainer's batch: taxels rand * 8, raw target rand * 250 at 100 x 100, both scaled by 2^exp."""
    g = torch.Generator().manual_seed(SEED + seed)
    s = 2.0 ** exp
    return torch.rand(B, 3, 4, 4, generator=g) * 8 * s, torch.rand(B, 1, 100, 100, generator=g) * 250 * s


def state_dict0(cfg=CFG, seed=SEED):
    return GC.step_data(cfg, 1, seed)[0]


# ------------------------------------------------------------------------------------------------------------ no GPU
def stem_amax_exponents(sd, sf=SF, B=4):
    """floor(log2 max|x|) of the pattern stem's first conv output (what the stem kernel publishes into its max|x| slot) for
    every rung of the ladder, on the CPU."""
    out = []
    for i, k in enumerate(LADDER):
        LR = raw_batch(B, 300 + i, k)[0]
        z = F.conv2d(F.interpolate(LR.double(), scale_factor=sf, mode="bilinear", align_corners=False),
                     sd["inputLayer_pattern_list.0.1.weight"].double(), padding=1)
        out.append(math.floor(math.log2(float(z.abs().max()))))
    return out


def test_the_ladder_crosses_power_of_two_buckets():
    """The amplitude ladder moves the stem's max|x| over at least four power-of-two buckets between consecutive replays, up
    and down: a scale or a slot kept from the capture or from the replay before lands in another bucket."""
    e = stem_amax_exponents(state_dict0())
    steps = [b - a for a, b in zip(e, e[1:])]
    assert max(e) - min(e) >= 4 and all(abs(s) >= 4 for s in steps), (e, steps)
    assert max(steps) > 0 > min(steps)
    # and the fp16x3 scale 2^(13 - e) differs accordingly
    assert len({13 - v for v in e}) >= 3, e


# ------------------------------------------------------------------------------------------------------------ TactileSR train
def train_call(m, opt, LR, HR, keep_grads=False):
    """One training step: forward (taxels asking for their gradient), loss, zero_grad, backward, Adam."""
    x = LR.cuda().requires_grad_()
    out = m(x)
    loss = Fh.mse_loss(out, HR.cuda())
    opt.zero_grad(set_to_none=not keep_grads)
    loss.backward()
    res = {"out": out, "loss": loss, "grad:LR": x.grad}
    res.update({k: v.clone() for k, v in model_state(m).items() if k.startswith("grad:")})
    opt.step()
    res.update({k: v for k, v in model_state(m).items() if not k.startswith("grad:")})
    res.update(opt_state(opt, m))
    return res


def new_adam(m):
    # (lr 1e-5: Adam moves every weight by +-lr whatever its gradient; a few steps at 1e-3 on these random weights push the
    #  whole output below the last ReLU, and two dead networks agree trivially)
    return optim.Adam(m.parameters(), lr=1e-5, weight_decay=1e-2)


def assert_live(res, label):
    """The call computed something: a non-zero output and (a train call) non-zero gradients nearly everywhere."""
    assert float(res["out"].detach().abs().max()) > 0, f"{label}: the output is all zero"
    grads = [v for k, v in res.items() if k.startswith("grad:")]
    assert sum(float(g.abs().max()) > 0 for g in grads) >= 0.9 * len(grads), f"{label}: dead gradients"


def fresh_trainer(m, opt):
    """A new module and a new optimizer with the state of `m` and `opt` (no gradients, no arena, no tables)."""
    f = fresh_like(m)
    fo = new_adam(f)
    fo.load_state_dict(copy.deepcopy(opt.state_dict()))
    return f, fo


SCENARIOS = {
    # (kind, B, options) per call
    "batch-sizes": [("train", 5, {}), ("train", 3, {}), ("train", 1, {}), ("train", 5, {})],
    "kept-grads": [("train", 5, {}), ("train", 3, {"keep_grads": True}), ("train", 1, {}), ("train", 5, {})],
    "eval-round-trip": [("train", 5, {}), ("train", 3, {}), ("eval", 3, {}), ("eval", 1, {}), ("train", 1, {}), ("train", 5, {})],
    "impl-switch": [("train", 5, {}), ("train", 3, {}), ("switch", 0, {}), ("train", 1, {}), ("train", 5, {})],
}
OTHER_IMPL = {"fp16x3": "bf16", "bf16": "fp16x3"}


@gpu
@pytest.mark.parametrize("scenario", list(SCENARIOS))
@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_tactilesr_train_history(impl, scenario):
    m = tsr_model(CFG, state_dict0(), train_impl=impl).train()
    if impl == "bf16":
        m.conv_impl = "bf16"
    opt = new_adam(m)
    for i, (kind, B, kw) in enumerate(SCENARIOS[scenario]):
        label = f"{scenario} call {i} ({kind} B={B})"
        if kind == "switch":
            m.train_impl = OTHER_IMPL[impl]
            continue
        LR, HR = batch(B, 10 + i)
        f, fo = fresh_trainer(m, opt)
        if kind == "eval":
            m.eval()
            want = {"out": f.eval()(LR.cuda())}
            assert_live(want, label)
            same_results({"out": m(LR.cuda())}, want, label)
            m.train()
            continue
        got, want = train_call(m, opt, LR, HR, **kw), train_call(f, fo, LR, HR)
        assert_live(want, label)
        same_results(got, want, label)


# ------------------------------------------------------------------------------------------------------------ TactileSR eval
ALL_IMPLS = ("fp16x3", "bf16x6", "f32", "bf16x3", "bf16")


@gpu
def test_tactilesr_eval_history():
    """B = 5, 1, 3; conv_impl through all five and back; parameter and statistics edits between calls."""
    m = tsr_model(CFG, state_dict0()).eval()

    def call(B, seed, label):
        LR, _ = batch(B, seed)
        want = {"out": fresh_like(m)(LR.cuda())}
        assert_live(want, label)
        same_results({"out": m(LR.cuda())}, want, label)
    for i, B in enumerate((5, 1, 3)):
        call(B, 40 + i, f"B={B}")
    for i, impl in enumerate(ALL_IMPLS + ALL_IMPLS[-2::-1]):
        m.conv_impl = impl
        call((3, 1, 5)[i % 3], 50 + i, f"conv_impl {impl} (call {i})")
    for i, flags in enumerate([(False, True), (True, False), (False, False), (True, True)]):
        m.fuse_pair, m.fuse_1x1 = flags
        call(3, 60 + i, f"fuse_pair, fuse_1x1 = {flags}")
    with torch.no_grad():
        m.output_layer[2].weight.mul_(2.0)
    call(3, 70, "after output_layer.2.weight.mul_")
    with torch.no_grad():
        m.patternFeatureExtra_layer[1].conv_5_2[1].running_var.add_(0.25)
        m.forceFeatureExtra_layer[0].conv1.bias.add_(0.1)
    call(1, 71, "after a running_var and a bias edit")
    m.head_impl = "f32"
    call(5, 72, "head_impl f32")


# ------------------------------------------------------------------------------------------------------------ blocks
BLOCK_CALLS = [(3, 8, 8), (2, 5, 7), (3, 8, 8)]


@gpu
@pytest.mark.parametrize("impl", BC.IMPLS)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_standalone_block_history(kind, impl):
    blk, _ = BC.make_block(kind)
    blk = blk.cuda()
    blk.conv_impl = blk.train_impl = impl
    for mode in ("eval", "train", "eval"):
        blk.train(mode == "train")
        for i, (B, H, W) in enumerate(BLOCK_CALLS):
            x, dy = BC.block_data(kind, B, H, W, seed=BC.SEED + 10 * i)
            f = fresh_like(blk)
            label = f"{kind} {impl} {mode} call {i} {(B, H, W)}"
            if mode == "eval":
                want = {"out": f(x.cuda())}
                assert_live(want, label)
                same_results({"out": blk(x.cuda())}, want, label)
                continue
            res = []
            for mod in (blk, f):
                mod.zero_grad()
                xin = x.cuda().requires_grad_()
                y = mod(xin)
                y.backward(dy.cuda())
                res.append({"out": y, "grad:x": xin.grad, **model_state(mod)})
            assert_live(res[1], label)
            same_results(res[0], res[1], label)


# ------------------------------------------------------------------------------------------------------------ tPSFNet
def tpsf_batch(B, seed):
    g = torch.Generator().manual_seed(SEED + seed)
    x = torch.rand(B, 3, 4, 4, generator=g) * 8
    depth = torch.rand(B, 100, 100, generator=g) * 3
    depth[0, 40:60, 30:70] = 4.0
    return x.cuda(), depth.cuda()


def tpsf_loss(net, x, depth):
    HR, LRd, psf, ab = net(x, depth)
    return F.mse_loss(x[:, 2:3], LRd) + 1e-3 * ab.sum(), {"out:HR": HR, "out:LRd": LRd, "out:ab": ab}


def tpsf_fresh(net):
    f = tactilesr_amd.tPSFNet(net.gama, net.perception_scale)
    f.load_state_dict(net.state_dict())
    f = f.cuda()
    for p, q in zip(net.parameters(), f.parameters()):
        q.grad = None if p.grad is None else p.grad.detach().clone()      # the same state: an accumulating step adds to these
    return f


TPSF_CALLS = [("direct", 600), ("accumulate", 20), ("twice", 20), ("direct", 600), ("direct", 20), ("accumulate", 600)]


@gpu
def test_tpsfnet_history():
    """B = 600, 20, 600 (split-K ns 32, 2, 32): a direct step, an accumulating step and a module applied twice in one graph
    in between, with Adam stepping after each."""
    torch.manual_seed(SEED + 80)
    net = tactilesr_amd.tPSFNet(0.5, 1.0).cuda()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    for i, (kind, B) in enumerate(TPSF_CALLS):
        f = tpsf_fresh(net)
        res = []
        for mod in (net, f):
            if kind != "accumulate":
                mod.zero_grad()
            x, depth = tpsf_batch(B, 90 + i)
            loss, outs = tpsf_loss(mod, x, depth)
            if kind == "twice":
                x2, depth2 = tpsf_batch(B, 190 + i)
                loss2, outs2 = tpsf_loss(mod, x2, depth2)
                loss = loss + loss2
                outs.update({k + "#2": v for k, v in outs2.items()})
            loss.backward()
            res.append({**outs, "loss": loss, **model_state(mod)})
        assert_live({"out": res[1]["out:LRd"], **res[1]}, f"tPSFNet call {i}")
        same_results(res[0], res[1], f"tPSFNet call {i} ({kind} B={B})")
        opt.step()


# ------------------------------------------------------------------------------------------------------------ graph replays
def trainer_config():
    return dict(TR.default_config(), scale_factor=SF)


@gpu
@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_graphed_train_step_over_the_amplitude_ladder(impl):
    """B = 4; one eager warm-up step, then the capture and a replay per rung (x 1, 2^5, 2^-5, 1): each against eager."""
    conf = trainer_config()
    sd = state_dict0()
    me, mg = (tsr_model(CFG, sd, train_impl=impl).train() for _ in range(2))
    oe, og = new_adam(me), new_adam(mg)
    ee, eg = WeightEMA(me, decay=0.9), WeightEMA(mg, decay=0.9)
    step = GraphedTrainStep(mg, og, dict(conf), warmup=1, ema=eg)
    for i, k in enumerate((0,) + LADDER):
        b = tuple(t.cuda() for t in raw_batch(4, 300 + max(i - 1, 0) + (100 if i == 0 else 0), k))
        pe = TR.train_one_iter(me, oe, b, conf, ema=ee)
        pg = step(b)
        label = f"{impl} call {i} (x 2^{k})"
        assert_live({"out": pe["total_loss"], **model_state(me)}, label)
        same_results({"loss:" + n: v for n, v in pg.items()}, {"loss:" + n: v for n, v in pe.items()}, label)
        same_results({**model_state(mg), **opt_state(og, mg), **ema_state(eg)},
                     {**model_state(me), **opt_state(oe, me), **ema_state(ee)}, label)
    assert step.captures == 1


@gpu
@pytest.mark.parametrize("variant", [dict(conv_impl="fp16x3"), dict(conv_impl="fp16x3", fuse_pair=False, fuse_1x1=False),
                                     dict(conv_impl="bf16")], ids=["fp16x3", "fp16x3-unfused", "bf16"])
def test_graphed_forward_over_the_amplitude_ladder(variant):
    m = tsr_model(CFG, state_dict0(), **variant).eval()
    xs = [raw_batch(4, 300 + i, k)[0].cuda() for i, k in enumerate(LADDER)]
    gf = GraphedForward(m, xs[0])
    for i, x in enumerate(xs):
        want = {"out": m(x)}
        assert_live(want, f"rung {i}")
        same_results({"out": gf(x).clone()}, want, f"rung {i} (x 2^{LADDER[i]})")
    # one all-NaN frame: it stays in its frame, and the next replay is clean
    bad = xs[0].clone()
    bad[2] = float("nan")
    y, want = gf(bad).clone(), m(bad)
    keep = [0, 1, 3]
    assert bool(torch.isfinite(y[keep]).all()) and torch.equal(y[keep], want[keep])
    assert torch.equal(torch.isnan(y[2]), torch.isnan(want[2]))
    same_results({"out": gf(xs[1]).clone()}, {"out": m(xs[1])}, "the replay after the NaN frame")
    same_results({"out": gf(xs[0]).clone()}, {"out": fresh_like(m)(xs[0])}, "and the one after, against a fresh module")
    assert gf.captures == 1


# ------------------------------------------------------------------------------------------------------------ writers and caches
def srcnn():
    torch.manual_seed(SEED + 7)
    m = tactilesr_amd.TactileSRCNN()
    BC.randomise(m, SEED + 8)
    return m.cuda().eval()


def block():
    return BC.make_block("msrb")[0].cuda().eval()


def sr():
    return tsr_model(CFG, state_dict0()).eval()


MODULES = {"TactileSR": sr, "MSRB": block, "TactileSRCNN": srcnn}


def module_input(name, seed=0):
    g = torch.Generator().manual_seed(SEED + 400 + seed)
    if name == "MSRB":
        return (torch.randn(3, 64, 9, 8, generator=g) * 2).cuda()
    return (torch.rand(3, 3, 4, 4, generator=g) * 8).cuda()


def set_grads(m, seed):
    g = torch.Generator().manual_seed(SEED + 500 + seed)
    for p in m.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(p.device)


def w_inplace(m):
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.mul_(1.0 + 0.01 * (i % 5)).add_(0.003)
        for n, b in m.named_buffers():
            if n.endswith("running_var"):
                b.mul_(1.5)
            elif n.endswith("running_mean"):
                b.add_(0.05)


def w_load_state_dict(m):
    g = torch.Generator().manual_seed(SEED + 600)
    sd = {k: (v.detach().cpu() * (1 + 0.05 * torch.rand(v.shape, generator=g)) if v.is_floating_point() else v.detach().cpu() + 3)
          for k, v in m.state_dict().items()}
    m.load_state_dict(sd)


def w_sgd(m):
    set_grads(m, 1)
    torch.optim.SGD(m.parameters(), lr=0.05).step()


def w_adam(m):
    opt = optim.Adam(m.parameters(), lr=1e-2, weight_decay=1e-2)
    set_grads(m, 2)
    opt.step()
    set_grads(m, 3)
    opt.step()


def w_adam_clipped(m):
    opt = optim.Adam(m.parameters(), lr=1e-2)
    set_grads(m, 4)
    opt.step_clipped(0.5)


def w_ema_copy_to(m):
    e = WeightEMA(m, decay=0.5, buffers="ema")
    w_inplace(m)
    e.update()
    e.copy_to()


def w_half_float(m):
    m.half().float()


def w_reset_running_stats(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.reset_running_stats()


def w_data_edit_and_invalidate(m):
    for p in m.parameters():
        p.data.mul_(1.25)
    tactilesr_amd.invalidate_weight_packs()


def w_bn_eps(m):
    for i, mod in enumerate(b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)):
        mod.eps = (1e-3, 1e-1, 1e-5)[i % 3]


def w_train_forward(m):
    m.train()
    m(module_input("MSRB" if isinstance(m, tactilesr_amd.MSRB) else "TactileSR", 9))
    m.eval()


def w_recalibrate_bn(m):
    recalibrate_bn(m, [batch(3, 700 + i) for i in range(2)], trainer_config())


def w_graphed_train_replay(m):
    m.train()
    opt = new_adam(m)
    step = GraphedTrainStep(m, opt, trainer_config(), warmup=1)
    for i in range(3):
        step(tuple(t.cuda() for t in raw_batch(3, 800 + i)))
    assert step.captures == 1
    m.eval()


WRITERS = {"in-place under no_grad": w_inplace, "load_state_dict": w_load_state_dict, "torch.optim.SGD.step": w_sgd,
           "optim.Adam.step": w_adam, "optim.Adam.step_clipped": w_adam_clipped, "WeightEMA.copy_to": w_ema_copy_to,
           "half().float()": w_half_float, "reset_running_stats": w_reset_running_stats,
           ".data edit + invalidate_weight_packs": w_data_edit_and_invalidate, "bn.eps": w_bn_eps,
           "train forward": w_train_forward, "recalibrate_bn": w_recalibrate_bn, "GraphedTrainStep replay": w_graphed_train_replay}
TRAINABLE_ONLY = {"train forward": ("TactileSR", "MSRB"), "recalibrate_bn": ("TactileSR",),
                  "GraphedTrainStep replay": ("TactileSR",)}
WRITER_CASES = [(w, n) for w in WRITERS for n in MODULES if n in TRAINABLE_ONLY.get(w, tuple(MODULES))]


def check_fresh(m, gf, name, label, seed):
    """The module's (and the graph's) forward FIRST, on whatever its caches hold; only then the fresh module."""
    x = module_input(name, seed)
    got = {"out": m(x).clone()}
    got_graph = {"out": gf(x).clone()} if gf is not None else None
    want = {"out": fresh_like(m)(x)}
    assert_live(want, label)
    same_results(got, want, label + ": eval forward")
    if gf is not None:
        same_results(got_graph, want, label + ": GraphedForward")
    return want["out"]


@gpu
@pytest.mark.parametrize("writer,name", WRITER_CASES, ids=[f"{n}-{w}" for w, n in WRITER_CASES])
def test_a_writer_is_followed_by_a_fresh_forward(writer, name):
    """Packs exist (an eval forward and a captured GraphedForward ran), the writer changes parameters or statistics, and
    the next eval forward and the next GraphedForward call equal a freshly built module's."""
    m = MODULES[name]()
    gf = GraphedForward(m, module_input(name, 0)) if name == "TactileSR" else None
    before = check_fresh(m, gf, name, "before", 2)
    key, captures = m._param_key(), gf.captures if gf is not None else 0
    check_fresh(m, gf, name, "before (packs in place)", 1)
    assert m._plan is not None and m._param_key() == m._plan_key == key, "building a fresh module moved this module's key"
    assert gf is None or gf.captures == captures
    WRITERS[writer](m)
    assert not m.training
    after = check_fresh(m, gf, name, writer, 2)
    assert not torch.equal(after, before), "the writer changed nothing the forward reads"
    check_fresh(m, gf, name, writer + " (second call)", 3)


@gpu
@pytest.mark.parametrize("name", list(MODULES))
def test_weight_ema_applied_is_followed_by_a_fresh_forward(name):
    m = MODULES[name]()
    gf = GraphedForward(m, module_input(name, 0)) if name == "TactileSR" else None
    e = WeightEMA(m, decay=0.5, buffers="ema")
    check_fresh(m, gf, name, "before", 1)
    w_inplace(m)
    e.update()
    check_fresh(m, gf, name, "after update", 2)
    with e.applied():
        check_fresh(m, gf, name, "inside applied()", 3)
    check_fresh(m, gf, name, "after applied()", 4)
