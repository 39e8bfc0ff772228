"""GPU checks of frozen parameters in the train step: with part of the model at ``requires_grad_(False)`` the backward issues
only the launches its plan (tactilesr_amd.model._train.backward_plan) keeps, and everything it still produces is the
all-trainable step's bit for bit -- the launches that remain are unchanged and the kernels are deterministic.  Also the two
head data-gradient entry points against ``tsr_head_bwd``, the Seqs transplant flow with ``freeze=True`` (eager, clipped,
graphed) and standalone ``MSRB`` / ``ResBlock`` modules with a frozen conv."""
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

import tactilesr_amd
from oracle import tactilesr_oracle as O
from tactilesr_amd import ddp, optim
from tactilesr_amd.model import _train
from tactilesr_amd.model import tactileSR_model as M
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.checkpoint import model_param_init
from tactilesr_amd.train.graph import GraphedTrainStep

import _bucket_peer as BP
import _frozen as FZ

pytestmark = pytest.mark.gpu


def _cfg(sf, T, Mb, R=1):
    return dict(scale_factor=sf, seqsCnt=T, patternFeatureExtraLayerCnt=Mb, forceFeatureExtraLayerCnt=R)


def _data(cfg, B, seed):
    sf, T = cfg["scale_factor"], cfg["seqsCnt"]
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), seed)
    g = torch.Generator().manual_seed(seed + 1)
    LR = torch.rand(B, 3 * T, 4, 4, generator=g) * 8
    HR = torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25
    return sd, LR.cuda(), HR.cuda()


def _model(cfg, sd, impl):
    m = tactilesr_amd.TactileSR(**cfg)
    m.train_impl = impl
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _stats(m):
    return {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


_REF = {}


def _reference(cfg, B, impl, seed):
    """The all-trainable step (taxel gradient included) from the seeded state, computed once per configuration."""
    key = (tuple(sorted(cfg.items())), B, impl, seed)
    if key not in _REF:
        sd, LR, HR = _data(cfg, B, seed)
        m = _model(cfg, sd, impl)
        x = LR.clone().requires_grad_(True)
        F.mse_loss(m(x), HR).backward()
        torch.cuda.synchronize()
        _REF[key] = ({n: p.grad.clone() for n, p in m.named_parameters()}, x.grad.clone(), _stats(m))
    return _REF[key]


CASES = [(pat, 3, T, 3, 3, "fp16x3") for pat in FZ.PATTERNS for T in (1, 2)]
CASES += [("middle_msrb", 3, 1, 3, 3, "f32"), ("bn_only", 3, 2, 3, 3, "bf16x6"), ("trunk", 10, 1, 2, 4, "bf16")]


@pytest.mark.parametrize("pattern,sf,T,Mb,B,impl", CASES, ids=[f"{c[0]}-sf{c[1]}-T{c[2]}-{c[5]}" for c in CASES])
def test_frozen_step_is_the_all_trainable_step_minus_the_unneeded_launches(pattern, sf, T, Mb, B, impl):
    cfg = _cfg(sf, T, Mb)
    seed = 5100 + 10 * T + sf
    ref_grads, ref_dx, ref_stats = _reference(cfg, B, impl, seed)
    sd, LR, HR = _data(cfg, B, seed)
    m = _model(cfg, sd, impl)
    named = dict(m.named_parameters())
    want, want_dx = FZ.PATTERNS[pattern](list(named))
    for n, p in named.items():
        p.requires_grad_(n in want)
    plan = _train.backward_plan(T, Mb, 1, want, want_dx)
    x = LR.clone().requires_grad_(want_dx)
    loss = F.mse_loss(m(x), HR)
    with FZ.CallCounter(_train) as cc:
        loss.backward()
    torch.cuda.synchronize()
    # the launches of this backward are the plan's
    assert cc.counts == FZ.expected_calls(plan, want), (cc.counts, FZ.expected_calls(plan, want))
    if pattern == "head":
        assert cc.counts == Counter(head_bwd=1, wgrad=1, reduce_splits=2)          # no backward conv_ex at all
    if pattern == "trunk":       # output_layer.0, inputContact_layer.0 and one seq[4] per frame; every dgrad of the full step
        full = _train.backward_plan(T, Mb, 1, frozenset(named), False)
        assert cc.counts["wgrad"] == 2 + T and cc.counts["conv_ex"] == sum(r.kind == "dgrad" for r in full)
    if pattern == "all":
        # output_layer.0, two per ResBlock, five per MSRB, inputContact_layer.0, one seq[4] per frame
        assert cc.counts["wgrad"] == 1 + 2 + 5 * Mb + 1 + T and cc.counts["head_bwd"] == 1
    # every wanted gradient is the all-trainable step's, bit for bit; frozen parameters have none
    for n, p in named.items():
        if n in want:
            assert p.grad is not None and torch.equal(p.grad, ref_grads[n]), n
        else:
            assert p.grad is None, n
    if want_dx:
        assert torch.equal(x.grad, ref_dx)
    else:
        assert x.grad is None
    for k, v in _stats(m).items():
        assert torch.equal(v, ref_stats[k]), k
    eng = m.train_engine()
    if not want:
        assert eng.arena is None
        return
    # the arena holds the wanted parameters only, in production order, and the gradients live in it
    order = FZ.production_order(plan, want)
    assert eng.arena.names == order and set(order) == set(want)
    opt = optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-5)

    def step():
        out = F.mse_loss(m(LR), HR)
        opt.zero_grad()
        out.backward()
        opt.step()

    opt.step()
    builds = opt.table_builds
    for _ in range(3):
        step()
    arena = eng.arena
    assert arena.names == order
    for n in order:
        assert named[n].grad.data_ptr() == arena.flat.data_ptr() + 4 * arena.offsets[n], n
    assert opt.table_builds == builds == 1
    # one flag flipped: the arena is laid out again and the fused Adam builds exactly one new chunk table
    flip = named[order[len(order) // 2]]
    flip.requires_grad_(False)
    step()
    assert eng.arena is not arena and eng.arena.names == [n for n in order if named[n] is not flip]
    step()
    assert opt.table_builds == builds + 1


# ------------------------------------------------------------------------------------------------- tsr_head_dgrad[_b16]
@pytest.mark.parametrize("b16", [False, True])
@pytest.mark.parametrize("H,W", [(5, 7), (40, 40)])
@pytest.mark.parametrize("cin,h_ctot", [(64, 64), (64, 128), (128, 128), (128, 160)])
def test_head_dgrad_is_head_bwds_data_gradient_bit_for_bit(cin, h_ctot, H, W, b16):
    from tactilesr_amd import _lib
    from tactilesr_amd._lib import ptr, stream, c_int as I
    B, GUARD = 3, 64
    dz_ctot = h_ctot
    g = torch.Generator().manual_seed(H * 100 + W + cin + h_ctot + int(b16))
    h0 = F.relu(torch.randn(B, cin, H, W, generator=g))
    h0d = M.to_cb16(h0.cuda(), h_ctot, 0)
    w = (torch.randn(1, cin, 3, 3, generator=g) * 0.1).cuda()
    out = F.relu(torch.randn(B, 1, H, W, generator=g)).cuda()
    dout = torch.randn(B, 1, H, W, generator=g).cuda()
    dt = torch.bfloat16 if b16 else torch.float32
    h0d = h0d.to(dt)
    n = B * dz_ctot * H * W

    def fresh():          # NaN-prefilled, with guard elements behind the tensor
        return torch.full((n + GUARD,), float("nan"), device="cuda").to(dt), torch.full((1 + GUARD,), float("nan"), device="cuda")

    dz_a, am_a = fresh()
    dz_b, am_b = fresh()
    am_a[0] = am_b[0] = 0.0
    wslab = torch.empty(2, cin * 9, device="cuda")
    lib = _lib.load()
    if b16:
        assert lib.tsr_head_bwd_b16(ptr(dout), ptr(out), ptr(h0d), I(h_ctot), I(cin), ptr(w), ptr(dz_a), I(dz_ctot), ptr(wslab),
                                    I(2), I(B), I(H), I(W), stream()) == 0
        assert lib.tsr_head_dgrad_b16(ptr(dout), ptr(out), ptr(h0d), I(h_ctot), I(cin), ptr(w), ptr(dz_b), I(dz_ctot), I(B),
                                      I(H), I(W), stream()) == 0
    else:
        assert lib.tsr_head_bwd(ptr(dout), ptr(out), ptr(h0d), I(h_ctot), I(cin), ptr(w), ptr(dz_a), I(dz_ctot), ptr(wslab),
                                I(2), I(B), I(H), I(W), ptr(am_a), stream()) == 0
        assert lib.tsr_head_dgrad(ptr(dout), ptr(out), ptr(h0d), I(h_ctot), I(cin), ptr(w), ptr(dz_b), I(dz_ctot), I(B), I(H),
                                  I(W), ptr(am_b), stream()) == 0
    torch.cuda.synchronize()
    bits = torch.int16 if b16 else torch.int32
    assert torch.equal(dz_a.view(bits), dz_b.view(bits))                  # written values and untouched NaNs alike
    got = M.from_cb16(dz_b[:n].float().contiguous(), B, cin, H, W, dz_ctot, 0)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert bool(torch.isnan(dz_b[n:].float()).all())                      # guard elements
    if dz_ctot > cin:
        rest = M.from_cb16(dz_b[:n].float().contiguous(), B, dz_ctot - cin, H, W, dz_ctot, cin)
        assert bool(torch.isnan(rest).all())                              # channels past cin are not this launch's
    if not b16:
        assert torch.equal(am_a.view(torch.int32), am_b.view(torch.int32))
        assert float(am_b[0]) == float(got.abs().max()) and bool(torch.isnan(am_b[1:]).all())


# ------------------------------------------------------------------------------------------------------- the Seqs flow
_ModeLog = BP.SinkLog          # records which case every GradSink of a backward took (`modes`); shared with the bucket tests


def _seqs_flow(freeze, seed=77):
    """The reference's two-stage recipe (train/tactileSRSeqs_train.py:43-77): the optimizer is built BEFORE the transplant."""
    cfgT, cfg1 = _cfg(3, 2, 2), _cfg(3, 1, 2)
    sdT = O.random_state_dict(O.tactilesr_state_shapes(**cfgT), seed)
    sd1 = O.random_state_dict(O.tactilesr_state_shapes(**cfg1), seed + 1)
    m = _model(cfgT, sdT, "fp16x3")
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    model_param_init(m, sd1, lambda: tactilesr_amd.TactileSR(**cfg1), freeze=freeze)
    m.train()
    conf = TR.default_config()
    conf.update(scale_factor=3, seqsCnt=2)
    g = torch.Generator().manual_seed(seed + 2)
    batches = [((torch.rand(3, 6, 4, 4, generator=g) * 8).cuda(), (torch.rand(3, 1, 20, 20, generator=g) * 250).cuda())
               for _ in range(3)]
    return m, opt, conf, batches


def test_seqs_flow_with_frozen_transplant_eager_clipped_and_graphed():
    clip = 1.0
    # (A) freeze=True, the fused clipped step
    ma, oa, conf, batches = _seqs_flow(True)
    start = {n: p.detach().clone() for n, p in ma.named_parameters()}
    with _ModeLog() as log:
        for b in batches[:2]:
            TR.train_one_iter(ma, oa, b, conf, clip_grad_norm=clip)
            assert TR.fused_clip_applies(ma, oa)
    assert log.modes == ["first", "direct"], log.modes
    after2 = {n: p.detach().clone() for n, p in ma.named_parameters()}
    for n, p in ma.named_parameters():
        if FZ.is_trunk(n):
            assert p.grad is None and torch.equal(p, start[n]), n                  # transplanted: untouched, no gradient
        else:
            assert p.grad is not None and not torch.equal(p, start[n]), n          # the rest trains
    # (B) freeze=False (the reference's flow), torch's two calls over the same gradient set: the parameters that train
    mb, ob, _, _ = _seqs_flow(False)
    trained = [p for n, p in mb.named_parameters() if not FZ.is_trunk(n)]
    norms = []
    for b in batches[:2]:
        loss, _ = TR.train_cal_loss(mb, b, conf)
        ob.zero_grad()
        loss.backward()
        assert not TR.fused_clip_applies(mb, ob)                                   # stale transplanted gradients in the way
        norms.append(float(torch.nn.utils.clip_grad_norm_(trained, clip)))
        ob.step()
    print(f"[seqs flow] gradient norms before clipping {norms} (clip {clip})")
    assert min(norms) > clip                                                      # the clip is active in both steps
    diff = [n for n, p in mb.named_parameters() if not torch.equal(p.detach(), after2[n])]
    print(f"[seqs flow] parameters differing between the frozen fused flow and the two-call flow: {diff}")
    assert not diff
    # (C) the graphed clipped step accepts the frozen flow and gives the eager step's weights bit for bit
    TR.train_one_iter(ma, oa, batches[2], conf, clip_grad_norm=clip)
    mc, oc, _, _ = _seqs_flow(True)
    gstep = GraphedTrainStep(mc, oc, conf, warmup=1, clip_grad_norm=clip)
    for b in batches:
        gstep(b)
    assert gstep.captures == 1
    for (n, a), (_, c) in zip(ma.named_parameters(), mc.named_parameters()):
        assert torch.equal(a, c), n
    for (n, a), (_, c) in zip(ma.named_buffers(), mc.named_buffers()):
        assert torch.equal(a, c), n
    # a flag flipped after the capture: the graph is dropped and captured again
    dict(mc.named_parameters())["output_layer.0.weight"].requires_grad_(False)
    gstep(batches[0])
    gstep(batches[1])
    assert gstep.captures == 2
    # nothing left to train: refused
    for p in mc.parameters():
        p.requires_grad_(False)
    with pytest.raises(tactilesr_amd._lib.TactileSRHipError, match="requires grad"):
        gstep(batches[0])


# ------------------------------------------------------------------------------------------------- standalone blocks
BLOCKS = FZ.BLOCK_SUBSETS


@pytest.mark.parametrize("kind,frozen,x_grad", BLOCKS, ids=[f"{k}-{f[0]}-x{int(x)}" for k, f, x in BLOCKS])
def test_standalone_block_with_a_frozen_conv(kind, frozen, x_grad):
    cls = M.MSRB if kind == "msrb" else M.ResBlock
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(3, 64, 12, 12, generator=g).cuda()
    dy = torch.randn(3, 64, 12, 12, generator=g).cuda()

    def block():
        torch.manual_seed(9)
        return cls().cuda().train()

    ref = block()
    xr = x0.clone().requires_grad_(True)
    ref(xr).backward(dy)
    blk = block()
    named = dict(blk.named_parameters())
    want = frozenset(n for n in named if n not in frozen)
    for n in frozen:
        named[n].requires_grad_(False)
    plan = _train.block_backward_plan(kind, want, x_grad)
    x = x0.clone().requires_grad_(x_grad)
    y = blk(x)
    with FZ.CallCounter(_train) as cc:
        y.backward(dy)
    torch.cuda.synchronize()
    assert cc.counts == FZ.expected_calls(plan, want), (cc.counts, FZ.expected_calls(plan, want))
    full = _train.block_backward_plan(kind, frozenset(named), True)          # something is saved against the full backward
    saved = FZ.expected_calls(full, frozenset(named)) - cc.counts
    assert sum(saved.values()) > 0 and not (cc.counts - FZ.expected_calls(full, frozenset(named)))
    rg = dict(ref.named_parameters())
    for n, p in named.items():
        if n in want:
            assert torch.equal(p.grad, rg[n].grad), n
        else:
            assert p.grad is None, n
    assert (x.grad is None) if not x_grad else torch.equal(x.grad, xr.grad)
    for (k, a), (_, b) in zip(blk.named_buffers(), ref.named_buffers()):
        assert torch.equal(a, b), k
    assert blk.block_engine().arena.names == FZ.production_order(plan, want)
