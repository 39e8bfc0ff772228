"""GPU checks of eval-mode BatchNorm layers inside the train step (``bn.eval()`` under ``model.train()``,
``hold_bn_statistics``): the four new kernels one launch at a time against fp64, the whole step in every fp32-grade
arithmetic against the per-layer-mode fp64 reference of tests/_bn_modes.py (method of tests/_gradcheck.py), the train-engine
forward with every layer held against the inference kernels, the bf16-storage step against the fp16x3 step, the launch
counts of the Seqs case and the graph-captured step."""
import ctypes
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

import tactilesr_amd
from tactilesr_amd import optim
from tactilesr_amd._lib import call, ptr, stream
from tactilesr_amd.model import _train
from tactilesr_amd.model.tactileSR_model import hold_bn_statistics
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

import _bn_modes as BM
import _frozen as FZ
import _gradcheck as GC

pytestmark = pytest.mark.gpu

I, Fl = ctypes.c_int, ctypes.c_float
CFG = dict(scale_factor=3, seqsCnt=2, patternFeatureExtraLayerCnt=2, forceFeatureExtraLayerCnt=1)
SEED = 7300
GUARD = 1024


# ------------------------------------------------------------------------------------------------- the apply kernel
def _ulp(ref, mant):
    """Spacing of a format with `mant` explicit significand bits at |ref| (normal range)."""
    return torch.pow(2.0, torch.floor(torch.log2(ref.abs().double().clamp_min(2.0 ** -120))) - mant)


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 100, 321, 1600])
def test_bn_bwd_apply_eval_vs_fp64(HW, B, C, b16):
    """g[:, coff:coff+C] *= scale on a slice at a non-zero offset of a 256-channel CB16 buffer.  HW = 1: a single thread per
    channel quad; 100: under one sweep; 321: the first pixel past one 256 x 5-quad sweep; 1600: the network's own 40 x 40.
    fp32: the product of two fp32 numbers rounded once (<= 1 ulp of the fp64 product), out_amax = the true maximum; bf16:
    the fp64 product rounded to bf16, within one bf16 ulp (the fp32 product is rounded a second time on the store).  Every
    other channel and a guard band on both sides hold NaN and must keep it; two launches agree bit for bit."""
    ctot, coff = 256, 48 if C == 64 else 80
    g = torch.Generator().manual_seed(HW * 31 + B * 7 + C)
    x = torch.randn(B, C, HW, generator=g) * torch.exp(torch.randn(B, C, HW, generator=g))
    scale = (torch.rand(C, generator=g) + 0.25) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    dt = torch.bfloat16 if b16 else torch.float32
    if b16:
        x = x.bfloat16().float()
    full = torch.full((B, ctot, HW), float("nan"))
    full[:, coff:coff + C] = x
    body = full.view(B, ctot // 16, 16, HW).permute(0, 1, 3, 2).contiguous().flatten().to(dt)
    nan = torch.full((GUARD,), float("nan"), dtype=dt)
    ref = x.double() * scale.double().view(1, C, 1)
    scale_d = scale.cuda()
    outs = []
    for _ in range(2):
        flat = torch.cat([nan, body, nan]).cuda()
        view = flat[GUARD:GUARD + body.numel()]
        if b16:
            call("tsr_bn_bwd_apply_eval_b16", ptr(view), I(ctot), I(coff), ptr(scale_d), I(C), I(B), I(HW), stream())
            am = None
        else:
            am = torch.zeros(1, device="cuda")
            call("tsr_bn_bwd_apply_eval", ptr(view), I(ctot), I(coff), ptr(scale_d), I(C), I(B), I(HW), ptr(am), stream())
        torch.cuda.synchronize()
        outs.append((flat.cpu(), None if am is None else am.cpu()))
    flat = outs[0][0]
    assert torch.equal(flat.view(torch.int16 if b16 else torch.int32), outs[1][0].view(torch.int16 if b16 else torch.int32))
    assert bool(flat[:GUARD].isnan().all()) and bool(flat[GUARD + body.numel():].isnan().all())
    got_full = flat[GUARD:GUARD + body.numel()].float().view(B, ctot // 16, HW, 16).permute(0, 1, 3, 2).reshape(B, ctot, HW)
    other = torch.ones(ctot, dtype=torch.bool)
    other[coff:coff + C] = False
    assert bool(got_full[:, other].isnan().all())
    got = got_full[:, coff:coff + C].double()
    assert bool(got.isfinite().all())
    if b16:
        target = ref.float().bfloat16().double()
        assert bool(((got - target).abs() <= _ulp(ref, 7)).all()), float(((got - target).abs() / _ulp(ref, 7)).max())
    else:
        assert bool(((got - ref).abs() <= _ulp(ref, 23)).all()), float(((got - ref).abs() / _ulp(ref, 23)).max())
        assert torch.equal(outs[0][1], outs[1][1]) and float(outs[0][1]) == float(got.abs().max())


# ---------------------------------------------------------------------------------------- the vector and finalize kernels
def _close(got, ref, rel=1e-6):
    got, ref = got.detach().cpu().double(), ref.double()
    return bool(((got - ref).abs() <= rel * ref.abs() + 1e-37).all())


@pytest.mark.parametrize("case", ["random", "var0", "nobias"])
@pytest.mark.parametrize("C", [16, 64, 128, 208])
def test_bn_eval_vectors_vs_fp64(C, case):
    """scale, shift, xhat_a, xhat_b from the running statistics: fp32 roundings of double arithmetic, 1e-6 relative per
    element; running_var = 0 (invstd = 1 / sqrt(eps)) and a conv without bias included; nothing is written but the four
    vectors; two launches agree bit for bit."""
    g = torch.Generator().manual_seed(C + len(case))
    bias = None if case == "nobias" else torch.randn(C, generator=g) * 0.1
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    if case == "var0":
        rv[::3] = 0.0
    eps = 1e-5
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    invstd = 1.0 / torch.sqrt(rv.double() + eps32)
    d = (bias.double() if bias is not None else 0.0) - rm.double()
    ref = [gamma.double() * invstd, beta.double() + d * gamma.double() * invstd, invstd, d * invstd]
    dev = [None if t is None else t.cuda() for t in (bias, gamma, beta, rm, rv)]
    keep = [None if t is None else t.clone() for t in dev]
    res = []
    for _ in range(2):
        vec = torch.full((4, C), float("nan"), device="cuda")
        call("tsr_bn_eval_vectors", *[ptr(t) for t in dev], Fl(eps), I(C), *[ptr(vec[i]) for i in range(4)], stream())
        torch.cuda.synchronize()
        res.append(vec.cpu())
    assert torch.equal(res[0], res[1])
    for i, name in enumerate(("scale", "shift", "xhat_a", "xhat_b")):
        assert _close(res[0][i], ref[i]), (name, float(((res[0][i].double() - ref[i]).abs() / ref[i].abs().clamp_min(1e-30)).max()))
    for a, b in zip(dev, keep):
        assert a is None or torch.equal(a, b)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("entries", [1, 7, 1030, 2400])
def test_bn_bwd_finalize_eval_vs_fp64(entries, C):
    """dgamma = sum over the slab entries of the g*xhat partials, dbeta = of the g partials (slab[entry][C][2] = {sum g,
    sum g*xhat}, the dgrad epilogue's format): double accumulation rounded to fp32, 1e-6 relative per element; entry counts
    below, at and beyond the 512 x (256 / C) entries one sweep of the reduction covers; two launches agree bit for bit."""
    g = torch.Generator().manual_seed(entries + C)
    slab = (torch.rand(entries, C, 2, generator=g) - 0.2) * torch.exp(torch.randn(entries, C, 2, generator=g))
    ref = slab.double().sum(0)
    slab_d = slab.cuda()
    res = []
    for _ in range(2):
        dg, db = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        work = torch.empty(512 * C * 3, dtype=torch.float64, device="cuda")
        call("tsr_bn_bwd_finalize_eval", ptr(slab_d), I(entries), I(C), ptr(dg), ptr(db), ptr(work), stream())
        torch.cuda.synchronize()
        res.append((dg.cpu(), db.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert _close(res[0][1], ref[:, 0]) and _close(res[0][0], ref[:, 1])
    # and the same numbers as the batch-statistics finalize hands out for dgamma / dbeta
    one = torch.ones(C, device="cuda")
    o = torch.empty(5, C, device="cuda")
    call("tsr_bn_bwd_finalize", ptr(slab_d), I(entries), I(C), ctypes.c_double(64.0), ptr(one), ptr(one), ptr(one), ptr(o[0]),
         ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4]), ptr(work), stream())
    assert torch.equal(o[0].cpu(), res[0][0]) and torch.equal(o[1].cpu(), res[0][1])


# ------------------------------------------------------------------------------------------------------- whole steps
_CACHE = {}


def _case(cfg, B, pattern, seed=SEED):
    """(state dict, LR, HR, CPU module in the pattern's modes, its recorded fp64 step), computed once per (cfg, B, pattern)."""
    key = (tuple(sorted(cfg.items())), B, pattern, seed)
    if key not in _CACHE:
        sd, LR, HR = GC.step_data(cfg, B, seed)
        cpu = tactilesr_amd.TactileSR(**cfg)
        cpu.load_state_dict(sd, strict=True)
        BM.set_modes(cpu, BM.pattern_paths(cpu, pattern))
        _CACHE[key] = (sd, LR, HR, cpu, BM.step(cpu, LR, HR, record=True))
    return _CACHE[key]


def _device_model(cfg, sd, impl, pattern):
    m = tactilesr_amd.TactileSR(**cfg)
    m.train_impl = impl
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    held = BM.pattern_paths(m, pattern)
    BM.set_modes(m, held)
    if pattern == "seqs":           # the Seqs recipe: the transplanted containers are frozen as well
        for n, p in m.named_parameters():
            p.requires_grad_(not FZ.is_trunk(n))
    return m, set(held)


def _stats(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


def _check_stats(before, after, held, ns_ref, tol):
    """Held layers: bit-identical; training layers: within `tol` of the reference, counter + 1."""
    for k, v in after.items():
        layer = k.rsplit(".", 1)[0]
        if layer in held:
            assert torch.equal(v, before[k]), f"{k}: a held layer's statistics moved"
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1 == int(ns_ref[k]), k
        else:
            assert GC.relerr(v, ns_ref[k]) < tol, (k, GC.relerr(v, ns_ref[k]))


@pytest.mark.parametrize("impl", ["fp16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("pattern", ["all", "seqs", "mixed", "stem"])
def test_train_step_with_held_layers_vs_fp64(pattern, impl):
    """B = 3 at 12 x 12 (a ragged 64-pixel tile, an odd batch against the 4-image workgroups): loss within 1e-5 of the
    per-layer-mode fp64 reference, the ReLU pattern equal up to rounding-zero flips, every parameter gradient (the conv biases
    in front of held layers included: no longer zero) within 1e-5 max-norm of the fp64 gradient on the device's pattern, held
    statistics bit-identical, training statistics within 1e-5."""
    sd, LR, HR, cpu, (l64, _, ns64, pre64, _) = _case(CFG, 3, pattern)
    m, held = _device_model(CFG, sd, impl, pattern)
    eng = m.train_engine()
    eng.keep_ctx = True
    before = _stats(m)
    out = m(LR.cuda())
    loss = F.mse_loss(out, HR.cuda())
    print(f"[{pattern} {impl}] loss {loss.item():.8g} vs {l64:.8g} ({abs(loss.item() - l64) / abs(l64):.2e})")
    assert abs(loss.item() - l64) < 1e-5 * abs(l64)
    loss.backward()
    torch.cuda.synchronize()
    _check_stats(before, _stats(m), held, ns64, 1e-5)
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    flips = GC.check_pattern(masks, pre64)
    _, g64m, _, _, _ = BM.step(cpu, LR, HR, masks=masks)
    want = {n for n, p in m.named_parameters() if p.requires_grad}
    for n, p in m.named_parameters():
        assert (p.grad is not None) == (n in want), n
    worst = GC.check_grads({n: p.grad for n, p in m.named_parameters() if n in want}, {k: v for k, v in g64m.items() if k in want},
                           tol=1e-5)
    print(f"[{pattern} {impl}] {flips} ReLU flips; worst on-pattern gradient error {worst[0]:.2e} ({worst[1]})")
    if pattern == "all":         # the bias in front of a held BatchNorm gets a real gradient, and the device has it
        k = "patternFeatureExtra_layer.1.conv_5_2.0.bias"
        assert float(g64m[k].abs().max()) > 1e-6 and float(m.get_parameter(k).grad.abs().max()) > 0


def test_train_step_seqs_pattern_taxel_gradient_sf10():
    """scale_factor 10 (40 x 40, the network's own size), B = 2, the Seqs pattern, LR.requires_grad_(): the taxel gradient and
    every wanted parameter gradient within 1e-5 of the fp64 reference on the device's pattern."""
    cfg = dict(CFG, scale_factor=10)
    sd, LR, HR, cpu, (l64, _, ns64, pre64, _) = _case(cfg, 2, "seqs")
    m, held = _device_model(cfg, sd, "fp16x3", "seqs")
    eng = m.train_engine()
    eng.keep_ctx = True
    before = _stats(m)
    x = LR.cuda().requires_grad_(True)
    loss = F.mse_loss(m(x), HR.cuda())
    assert abs(loss.item() - l64) < 1e-5 * abs(l64)
    loss.backward()
    torch.cuda.synchronize()
    _check_stats(before, _stats(m), held, ns64, 1e-5)
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    GC.check_pattern(masks, pre64)
    _, g64m, _, _, dx64 = BM.step(cpu, LR, HR, masks=masks, want_dx=True)
    want = {n for n, p in m.named_parameters() if p.requires_grad}
    GC.check_grads({n: p.grad for n, p in m.named_parameters() if n in want}, {k: v for k, v in g64m.items() if k in want}, tol=1e-5)
    e = GC.relerr(x.grad, dx64)
    print(f"[seqs sf10] taxel gradient error {e:.2e}")
    assert e < 1e-5


@pytest.mark.parametrize("impl", ["fp16x3", "bf16x6", "f32"])
def test_all_held_forward_equals_the_inference_path(impl):
    """Two independent paths: with all BatchNorm layers held the train engine's forward (raw conv outputs + running-statistics
    vectors applied by the consumers) computes what model.eval() computes on the inference kernels (folded BatchNorm)."""
    sd, LR, HR, _, _ = _case(CFG, 3, "all")
    m, held = _device_model(CFG, sd, impl, "all")
    m.conv_impl = impl
    assert len(held) == 13 and m.training
    before = _stats(m)
    with torch.no_grad():
        y_train = m(LR.cuda()).clone()
        y_eval = m.eval()(LR.cuda())
    for k, v in _stats(m).items():
        assert torch.equal(v, before[k]), k
    e = GC.relerr(y_train, y_eval)
    print(f"[all held {impl}] train-engine forward vs inference path {e:.2e}")
    assert e < 1e-5


# ------------------------------------------------------------------------------------------------------- bf16 storage
def _grads_of(cfg, sd, LR, HR, impl, pattern):
    m, held = _device_model(cfg, sd, impl, pattern)
    before = _stats(m)
    F.mse_loss(m(LR.cuda()), HR.cuda()).backward()
    torch.cuda.synchronize()
    after = _stats(m)
    for k in after:
        if k.rsplit(".", 1)[0] in held:
            assert torch.equal(after[k], before[k]), k
    return {n: p.grad.detach().cpu().double().flatten() for n, p in m.named_parameters() if p.grad is not None}, m


def _distance(got, ref):
    """Worst 1 - cosine and |norm ratio - 1| over the parameters whose reference gradient is not zero + noise (conv biases in
    front of a train-mode BatchNorm, as in tests/_gradcheck.bf16_train_step_vs_emulating_oracle)."""
    top = max(float(v.abs().max()) for v in ref.values())
    dc, dn = (-1.0, ""), (-1.0, "")
    for k, r in ref.items():
        if float(r.abs().max()) < 1e-6 * top:
            continue
        g = got[k]
        dc = max(dc, (1.0 - float(g @ r / (g.norm() * r.norm()).clamp_min(1e-300)), k))
        dn = max(dn, (abs(float(g.norm() / r.norm()) - 1.0), k))
    print(f"    worst 1-cos {dc[0]:.3e} ({dc[1]}), worst |ratio-1| {dn[0]:.3e} ({dn[1]})")
    return dc[0], dn[0]


_BF16_BASE = {}


@pytest.mark.parametrize("pattern", ["all", "seqs", "mixed"])
def test_bf16_storage_step_with_held_layers_stays_at_the_all_training_distance(pattern):
    """The oracle's bf16 emulation has the train step's rounding points only in training mode, so there is no emulating
    reference for a held layer.  Instead: the distance of the bf16-storage step from the fp16x3 step (worst 1 - cosine and
    worst |norm ratio - 1| over the parameter gradients) is measured first on the unchanged all-training code, then for the
    held pattern against the same pattern in fp16x3; a held pattern must stay within 1.5x the all-training distance (the
    margin covers the missing batch-statistics terms, which average rounding noise out; a wrong vector or a missing scale
    shows as tens of percent).  Held statistics are bit-identical, and pattern "all" reaches the bf16 pair launch."""
    sd, LR, HR, _, _ = _case(CFG, 3, "none")
    if not _BF16_BASE:
        ref, _ = _grads_of(CFG, sd, LR, HR, "fp16x3", "none")
        got, _ = _grads_of(CFG, sd, LR, HR, "bf16", "none")
        _BF16_BASE["d"] = _distance(got, ref)
    base_c, base_n = _BF16_BASE["d"]
    ref, _ = _grads_of(CFG, sd, LR, HR, "fp16x3", pattern)
    got, m = _grads_of(CFG, sd, LR, HR, "bf16", pattern)
    assert set(got) == set(ref)
    eng = m.train_engine()
    assert eng.io16 and eng._b16k(128, 64, 5)          # the stage-1 pair of every MSRB runs the one-launch bf16 form
    dc, dn = _distance(got, ref)
    print(f"[bf16 vs fp16x3] all training: 1-cos {base_c:.3e}, |ratio-1| {base_n:.3e}; {pattern}: 1-cos {dc:.3e}, |ratio-1| {dn:.3e}")
    # measured on MI355X (this model and batch), worst parameter gradient as (1 - cosine, |norm ratio - 1|):
    #   all training (the baseline)  7.46e-2, 1.087e-1   -> bar 1.12e-1, 1.63e-1
    #   all held                     2.20e-3, 3.86e-2
    #   trunk held and frozen        2.06e-2, 4.54e-2
    #   mixed inside one MSRB        8.11e-2, 8.47e-2
    assert dc <= 1.5 * base_c and dn <= 1.5 * base_n, (pattern, dc, base_c, dn, base_n)


# ------------------------------------------------------------------------------------------------------ launch counts
class _Names:
    """Counts what `_train.call` / `_train.conv_ex` are asked to launch, by entry-point name (they stay in effect)."""

    def __init__(self):
        self.names, self.conv = Counter(), []

    def __enter__(self):
        self._call, self._conv_ex = _train.call, _train.conv_ex

        def call_(name, *args):
            self.names[name] += 1
            return self._call(name, *args)

        def conv_ex(**kw):
            self.conv.append((kw.get("epi_mode", 0), bool(kw.get("bn"))))
            return self._conv_ex(**kw)

        _train.call, _train.conv_ex = call_, conv_ex
        return self

    def __exit__(self, *exc):
        _train.call, _train.conv_ex = self._call, self._conv_ex
        return False


def _prefix(names, *prefixes):
    return sum(v for k, v in names.items() if k.startswith(prefixes))


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_launch_counts_of_the_seqs_case_and_of_the_unchanged_step(impl):
    """Seqs pattern with the trunk frozen: no statistics launch for a trunk layer in forward (the finalize / cb16_stats calls
    left are the 2T + 1 non-trunk layers'), no tsr_bn_bwd_finalize* for one, exactly one tsr_bn_bwd_apply_eval* per trunk
    BatchNorm tensor the plan keeps (three per MSRB).  With every layer training the step calls what the plan without held
    layers implies -- the parent's counts -- and none of the new entry points."""
    T, Mb = CFG["seqsCnt"], CFG["patternFeatureExtraLayerCnt"]
    sd, LR, HR, _, _ = _case(CFG, 3, "none")
    b16 = "_b16" if impl == "bf16" else ""
    # ---- every layer training: the parent's launches
    m, _ = _device_model(CFG, sd, impl, "none")
    names = [n for n, _ in m.named_parameters()]
    with _Names() as fw:
        loss = F.mse_loss(m(LR.cuda()), HR.cuda())
    with FZ.CallCounter(_train) as cc, _Names() as bw:
        loss.backward()
    torch.cuda.synchronize()
    plan = _train.backward_plan(T, Mb, 1, frozenset(names), False)
    assert cc.counts == FZ.expected_calls(plan, frozenset(names))
    n_bn = 2 * T + 1 + 4 * Mb
    pair = Mb if impl == "bf16" else 0
    assert fw.names["tsr_bn_stats_finalize"] == n_bn - pair and fw.names["tsr_cb16_stats" + b16] == T
    assert sum(1 for e, _ in fw.conv if e == 1) == n_bn - T - pair
    assert bw.names["tsr_bn_bwd_finalize"] == bw.names["tsr_bn_bwd_apply" + b16] == 3 * Mb + 1 + 2 * T
    assert not _prefix(fw.names + bw.names, "tsr_bn_eval_vectors", "tsr_bn_bwd_finalize_eval", "tsr_bn_bwd_apply_eval")
    # ---- the Seqs case
    m, held = _device_model(CFG, sd, impl, "seqs")
    want = frozenset(n for n, p in m.named_parameters() if p.requires_grad)
    with _Names() as fw:
        loss = F.mse_loss(m(LR.cuda()), HR.cuda())
    with FZ.CallCounter(_train) as cc, _Names() as bw:
        loss.backward()
    torch.cuda.synchronize()
    assert fw.names["tsr_bn_stats_finalize"] == 2 * T + 1 and fw.names["tsr_cb16_stats" + b16] == T
    assert fw.names["tsr_bn_eval_vectors"] == (3 if impl == "bf16" else 4) * Mb
    assert sum(1 for e, _ in fw.conv if e == 1) == T + 1 + pair        # (the bf16 pair form only knows epi_mode 1)
    assert _prefix(bw.names, "tsr_bn_bwd_finalize") == bw.names["tsr_bn_bwd_finalize"] == 2 * T + 1
    assert bw.names["tsr_bn_bwd_apply_eval" + b16] == 3 * Mb == _prefix(bw.names, "tsr_bn_bwd_apply_eval")
    assert bw.names["tsr_bn_bwd_apply" + b16] == 2 * T + 1
    assert sum(1 for _, bn in bw.conv if bn) == 2 * T + 1
    plan = _train.backward_plan(T, Mb, 1, want, False, bn_eval=held)
    assert cc.counts == FZ.expected_calls(plan, want)


# -------------------------------------------------------------------------------------------------- GraphedTrainStep
def _graph_setup(impl="fp16x3"):
    torch.manual_seed(11)
    m = tactilesr_amd.TactileSR(**CFG).cuda().train()
    m.train_impl = impl
    with torch.no_grad():           # statistics that are not 0 / 1
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    for n, p in m.named_parameters():
        p.requires_grad_(not FZ.is_trunk(n))
    hold_bn_statistics(m.patternFeatureExtra_layer)
    hold_bn_statistics(m.forceFeatureExtra_layer)
    opt = optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2)
    conf = TR.default_config()
    conf.update(scale_factor=CFG["scale_factor"], seqsCnt=CFG["seqsCnt"])
    return m, opt, conf


def test_graphed_step_with_held_layers_is_bit_identical_and_recaptures():
    g = torch.Generator().manual_seed(3)
    batches = [((torch.rand(3, 6, 4, 4, generator=g) * 8).cuda(), (torch.rand(3, 1, 100, 100, generator=g) * 250).cuda())
               for _ in range(5)]
    ma, oa, conf = _graph_setup()
    mg, og, _ = _graph_setup()
    gstep = GraphedTrainStep(mg, og, conf, warmup=1)
    trunk = set(BM.trunk_bn_paths(ma))
    start = _stats(ma)

    def same(i):
        for (n, a), (_, b) in zip(ma.named_parameters(), mg.named_parameters()):
            assert torch.equal(a, b), (i, n)
            assert (a.grad is None) == (b.grad is None) and (a.grad is None or torch.equal(a.grad, b.grad)), (i, n)
        for (n, a), (_, b) in zip(ma.named_buffers(), mg.named_buffers()):
            assert torch.equal(a, b), (i, n)

    for i, b in enumerate(batches[:3]):          # eager warm-up, capture + replay, replay
        ma.train()
        mg.train()                               # the trainer's per-epoch model.train(): the marks survive it
        la = TR.train_one_iter(ma, oa, b, conf)["total_loss"].detach().clone()
        lg = gstep(b)["total_loss"].detach().clone()
        assert torch.equal(la, lg), (i, float(la), float(lg))
        same(i)
    assert gstep.captures == 1
    now = _stats(mg)
    for k, v in now.items():
        assert torch.equal(v, start[k]) == (k.rsplit(".", 1)[0] in trunk), k
    # one more layer held between calls: the capture is dropped, a new one matches again
    hold_bn_statistics(ma.inputContact_layer)
    hold_bn_statistics(mg.inputContact_layer)
    for i, b in enumerate(batches[3:], 3):
        la = TR.train_one_iter(ma, oa, b, conf)["total_loss"].detach().clone()
        lg = gstep(b)["total_loss"].detach().clone()
        assert torch.equal(la, lg), (i, float(la), float(lg))
        same(i)
    assert gstep.captures == 2
    for k, v in _stats(mg).items():
        if k.startswith("inputContact_layer.1."):
            assert torch.equal(v, now[k]), k
