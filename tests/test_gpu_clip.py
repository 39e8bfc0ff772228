"""GPU checks of gradient-norm clipping (the reference ``Trainer(clip_grad_norm=...)``, cpu/trainer.py:354-356:
``clip_grad_norm_(model.parameters(), c)`` between backward and the Adam step).

``optim.Adam.step_clipped`` (one ``tsr_grad_norm_multi`` + one ``tsr_adam_l2_multi_clip`` per set) against torch's own
``clip_grad_norm_`` arithmetic on the same gradients: the norm to a few ulps, the coefficient, the clipped gradients and
the step after it bit for bit; the clipped gradients and Adam moments against an fp64 oracle; ``train_one_iter``'s
fused and fallback paths; torch's NaN / Inf rules; the graphed step against the eager one; determinism; tPSFNet."""
import math

import pytest
import torch

import tactilesr_amd
from oracle import tactilesr_oracle as O
import _gradcheck as GC
from tactilesr_amd import optim
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep
from tactilesr_amd.train.lr_scheduler import LRWarmupScheduler

pytestmark = pytest.mark.gpu

B = 32


def _model(impl="fp16x3", seed=42):
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR().cuda().train()
    m.train_impl = impl
    return m


def _adam(params):
    return optim.Adam(params, lr=1e-3, weight_decay=1e-2)


def _batches(n, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (torch.rand(B, 1, 100, 100, generator=g) * 250).cuda())
            for _ in range(n)]


def _backward(m, batch, conf):
    """One real train-mode forward + backward: the gradients land in the engine's gradient arena."""
    for p in m.parameters():
        p.grad = None
    loss, _ = TR.train_cal_loss(m, batch, conf)
    loss.backward()
    assert all(p.grad is not None for p in m.parameters())


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _assert_same_step(ma, oa, mb, ob, grads=True):
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert _same(a.detach(), b.detach()), n
        if grads:
            assert _same(a.grad, b.grad), n
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]), n
        assert _same(sa["exp_avg"], sb["exp_avg"]) and _same(sa["exp_avg_sq"], sb["exp_avg_sq"]), n


def _twin_with_grads(m, grads, impl="fp16x3"):
    t = _model(impl)
    for p, g in zip(t.parameters(), grads):
        p.grad = g.clone()
    return t


@pytest.mark.parametrize("factor", [0.1, 10.0], ids=["active", "inactive"])
def test_norm_and_clipped_step_are_torchs(factor):
    conf = TR.default_config()
    m = _model()
    opt = _adam(m.parameters())
    _backward(m, _batches(1)[0], conf)
    g0 = [p.grad.detach().clone() for p in m.parameters()]
    ref = torch.nn.utils.get_total_norm(g0)
    n64 = math.sqrt(sum(float((g.double() ** 2).sum()) for g in g0))
    max_norm = factor * float(ref)

    launches = opt.launches
    norm = opt.step_clipped(max_norm)
    assert opt.launches - launches == 3 and opt.table_builds == 1          # 2 norm kernels + one Adam set
    assert norm.dim() == 0 and norm.is_cuda and norm.dtype == torch.float32
    print(f"[clip] norm {float(norm):.8e}  torch {float(ref):.8e}  fp64 {n64:.8e}")
    assert abs(float(norm) - float(ref)) <= 2e-6 * float(ref)
    assert abs(float(norm) - n64) <= 1e-6 * n64

    # the twin: the same gradients, torch's clip with OUR norm, then the plain step
    t = _twin_with_grads(m, g0)
    topt = _adam(t.parameters())
    torch.nn.utils.clip_grads_with_norm_(list(t.parameters()), max_norm, norm)
    topt.step()
    _assert_same_step(m, opt, t, topt)
    changed = any(not _same(p.grad, g) for p, g in zip(m.parameters(), g0))
    assert changed == (factor < 1)
    if factor > 1:       # inactive: the gradients are untouched and the step is the plain one
        assert all(_same(p.grad, g) for p, g in zip(m.parameters(), g0))
    else:                # active: the clipped gradients have norm max_norm
        after = float(torch.nn.utils.get_total_norm([p.grad for p in m.parameters()]))
        assert abs(after - max_norm) <= 1e-5 * max_norm


def test_clipped_step_vs_fp64_oracle():
    """The clipped gradients and the first Adam moment after the step against fp64: oracle gradients on the device's
    ReLU pattern (tests/_gradcheck.py), clipped in fp64, one fp64 Adam step.  Not judged by the weights: Adam's first
    step moves every weight by +-lr whatever |g'| is, so a step that never clipped would pass a weights-only check."""
    conf = TR.default_config()
    m = _model()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    eng = m.train_engine()
    eng.keep_ctx = True
    opt = _adam(m.parameters())
    LR, HR = _batches(1, seed=3)[0]
    _backward(m, (LR, HR), conf)
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    eng.keep_ctx, eng.last_ctx = False, None
    LRc = LR.cpu()[:, :3].float()
    HRc = O.prepare_target(HR.cpu(), conf["HR_scale_num"], conf["scale_factor"])
    _, g64, _, _ = GC.oracle_grads(sd, LRc, HRc, masks=masks)
    n64 = math.sqrt(sum(float((g ** 2).sum()) for g in g64.values()))
    max_norm = 0.1 * n64
    coef64 = min(max_norm / (n64 + 1e-6), 1.0)
    g64c = {k: g * coef64 for k, g in g64.items()}
    p64 = {k: v.double() for k, v in sd.items() if O.is_trainable(k)}
    state = {}
    O.adam_l2_step(p64, g64c, state, 1, 1e-3, 1e-2)

    opt.step_clipped(max_norm)
    named = dict(m.named_parameters())
    worst = GC.check_grads({k: p.grad for k, p in named.items()}, g64c, tol=1e-5)
    # exp_avg = (1 - beta1) (g' + wd w): its error is the clipped gradient's.  Where the exact gradient is 0 (a conv bias
    # in front of a train-mode BatchNorm) exp_avg is (1 - beta1) wd w plus the gradient's rounding noise, so it gets
    # the gradient check's absolute bar for those tensors, through the factor (1 - beta1).
    worst_m = 0.0
    for k, p in named.items():
        got, ref = opt.state[p]["exp_avg"].detach().cpu().double(), state[k]["m"]
        err = float((got - ref).abs().max())
        if float(g64c[k].abs().max()) < 1e-6:
            assert err < 0.1 * 1e-4, (k, err)
            continue
        rel = err / float(ref.abs().max())
        worst_m = max(worst_m, rel)
        assert rel <= 1e-5, (k, rel)
    print(f"[clip vs fp64] worst clipped-gradient error {worst[0]:.2e} ({worst[1]}), exp_avg {worst_m:.2e}")


def test_train_one_iter_fused_and_fallback_paths():
    conf = TR.default_config()
    batch = _batches(1, seed=5)[0]
    probe = _model()
    _backward(probe, batch, conf)
    c = 0.2 * float(torch.nn.utils.get_total_norm([p.grad for p in probe.parameters()]))
    del probe

    # fused: optim.Adam over the whole model
    ma = _model()
    oa = _adam(ma.parameters())
    TR.train_one_iter(ma, oa, batch, conf)            # step 1 plain: state and tables exist
    launches = oa.launches
    TR.train_one_iter(ma, oa, batch, conf, clip_grad_norm=c)
    assert oa.launches - launches == 3
    # ... equals backward + step_clipped, and torch's clip with that norm + the plain step
    mb, mc = _model(), _model()
    ob, oc = _adam(mb.parameters()), _adam(mc.parameters())
    for mm, oo in ((mb, ob), (mc, oc)):
        TR.train_one_iter(mm, oo, batch, conf)
        _backward(mm, batch, conf)
    norm = ob.step_clipped(c)
    torch.nn.utils.clip_grads_with_norm_(list(mc.parameters()), c, norm)
    oc.step()
    _assert_same_step(ma, oa, mb, ob)
    _assert_same_step(ma, oa, mc, oc)

    # fallback 1: torch.optim.Adam -- the reference's two calls
    def torch_adam(m):
        return torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    md, me = _model(), _model()
    od, oe = torch_adam(md), torch_adam(me)
    TR.train_one_iter(md, od, batch, conf, clip_grad_norm=c)
    _backward(me, batch, conf)
    torch.nn.utils.clip_grad_norm_(me.parameters(), c)
    oe.step()
    # fallback 2: optim.Adam holding part of the model (the rest still has gradients, and is clipped with them)
    mf, mg = _model(), _model()
    of, og = _adam(list(mf.parameters())[2:]), _adam(list(mg.parameters())[2:])
    launches = of.launches
    TR.train_one_iter(mf, of, batch, conf, clip_grad_norm=c)
    assert of.launches - launches == 1                # no norm kernels: torch's clip_grad_norm_, then the plain step
    _backward(mg, batch, conf)
    torch.nn.utils.clip_grad_norm_(mg.parameters(), c)
    og.step()
    for (ma_, oa_), (mb_, ob_) in (((md, od), (me, oe)), ((mf, of), (mg, og))):
        for (n, a), (_, b) in zip(ma_.named_parameters(), mb_.named_parameters()):
            assert _same(a.detach(), b.detach()) and _same(a.grad, b.grad), n
            if a in oa_.state:
                for k in ("exp_avg", "exp_avg_sq"):
                    assert _same(oa_.state[a][k], ob_.state[b][k]), (n, k)
    after = float(torch.nn.utils.get_total_norm([p.grad for p in mf.parameters()]))
    assert abs(after - c) <= 1e-5 * c                 # the fallback clipped over model.parameters()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradients_follow_torch(bad):
    conf = TR.default_config()
    m = _model()
    opt = _adam(m.parameters())
    _backward(m, _batches(1, seed=9)[0], conf)
    params = list(m.parameters())
    with torch.no_grad():
        params[3].grad.view(-1)[17] = bad                 # a data value in one arena view
    t = _twin_with_grads(m, [p.grad for p in params])
    tnorm = torch.nn.utils.clip_grad_norm_(t.parameters(), 1.0)
    norm = opt.step_clipped(1.0)
    if math.isnan(bad):
        assert math.isnan(float(norm)) and math.isnan(float(tnorm))
        assert all(torch.isnan(p.grad).all() for p in params)
    else:
        assert float(norm) == float(tnorm) == math.inf
        for i, p in enumerate(params):
            if i == 3:
                assert torch.isnan(p.grad.view(-1)[17]) and int(torch.isnan(p.grad).sum()) == 1
            finite = ~torch.isnan(p.grad)
            assert (p.grad[finite] == 0).all(), i
    for p, q in zip(params, t.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=0, atol=0, equal_nan=True)


def _sched(opt):
    return LRWarmupScheduler(torch.optim.lr_scheduler.StepLR(opt, 2, 0.8), epoch_len=4, warmup_t=8,
                             warmup_mode="auto", warmup_factor=1e-4)


def _run(step, sched, batches, start=0, on_step=None):
    losses = []
    for i, b in enumerate(batches, start):
        losses.append(step(b)["total_loss"].detach().clone())
        sched.iter_update()
        if (i + 1) % 4 == 0:
            sched.epoch_update()
        if on_step is not None:
            on_step(i)
    return losses


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
def test_graphed_clipped_trajectory_is_bit_identical_to_eager(impl):
    conf = TR.default_config()
    batches = _batches(16, seed=13)
    probe = _model(impl)
    _backward(probe, batches[0], conf)
    c = 0.2 * float(torch.nn.utils.get_total_norm([p.grad for p in probe.parameters()]))
    del probe

    me = _model(impl)
    oe = _adam(me.parameters())
    se = _sched(oe)
    active = []

    def clipped(i):      # after the step p.grad holds the clipped gradient: its norm is c exactly when clipping acted
        n = float(torch.nn.utils.get_total_norm([p.grad for p in me.parameters()]))
        active.append(n >= c * (1 - 1e-4))
    le = _run(lambda b: TR.train_one_iter(me, oe, b, conf, clip_grad_norm=c), se, batches[:12], on_step=clipped)
    assert sum(active) >= 8, active

    mg = _model(impl)
    og = _adam(mg.parameters())
    sg = _sched(og)
    gstep = GraphedTrainStep(mg, og, conf, warmup=1, clip_grad_norm=c)
    lg = _run(gstep, sg, batches[:12])
    assert gstep.captures == 1
    assert oe.launches == og.launches == 12 * 3
    for i, (x, y) in enumerate(zip(le, lg)):
        assert _same(x, y), (i, float(x), float(y))
    _assert_same_step(me, oe, mg, og)
    for (n, a), (_, b) in zip(me.named_buffers(), mg.named_buffers()):
        assert torch.equal(a, b), n

    # a new clip value is a baked constant: the graph is dropped, one eager step, then a new capture
    gstep.clip_grad_norm = 0.5 * c
    le = _run(lambda b: TR.train_one_iter(me, oe, b, conf, clip_grad_norm=0.5 * c), se, batches[12:], start=12)
    lg = _run(gstep, sg, batches[12:], start=12)
    assert gstep.captures == 2
    assert all(_same(x, y) for x, y in zip(le, lg))
    _assert_same_step(me, oe, mg, og)


def test_graphed_clip_refuses_a_partial_optimizer():
    conf = TR.default_config()
    m = _model()
    gstep = GraphedTrainStep(m, _adam(list(m.parameters())[1:]), conf, clip_grad_norm=1.0)
    with pytest.raises(tactilesr_amd._lib.TactileSRHipError, match="clip_grad_norm"):
        gstep(_batches(1)[0])


def test_clipped_step_is_deterministic():
    conf = TR.default_config()
    batch = _batches(1, seed=21)[0]
    runs = []
    for _ in range(2):
        m = _model()
        opt = _adam(m.parameters())
        _backward(m, batch, conf)
        n1 = opt.step_clipped(0.05).clone()
        _backward(m, batch, conf)
        n2 = opt.step_clipped(0.05).clone()
        runs.append((m, opt, n1, n2))
    (ma, oa, a1, a2), (mb, ob, b1, b2) = runs
    assert _same(a1, b1) and _same(a2, b2)
    _assert_same_step(ma, oa, mb, ob)


def test_tpsf_clipped_step_is_torchs():
    from tactilesr_amd.train import tPSFNet_train as TP

    def net():
        torch.manual_seed(4)
        return tactilesr_amd.tPSFNet(1.4, None).cuda()
    g = torch.Generator().manual_seed(2)
    batch = ((torch.rand(4, 3, 4, 4, generator=g) * 800).cuda(), (torch.rand(4, 100, 100, generator=g) > 0.7).float().cuda())
    a = net()
    loss, _ = TP.train_cal_loss(a, batch, 100.0)
    loss.backward()
    grads = [p.grad.detach().clone() for p in a.parameters()]
    assert grads
    ref = float(torch.nn.utils.get_total_norm(grads))
    max_norm = 0.1 * ref
    oa = _adam(a.parameters())
    norm = oa.step_clipped(max_norm)
    assert abs(float(norm) - ref) <= 2e-6 * ref
    t = net()
    for p, gr in zip(t.parameters(), grads):
        p.grad = gr.clone()
    ot = _adam(t.parameters())
    torch.nn.utils.clip_grads_with_norm_(list(t.parameters()), max_norm, norm)
    ot.step()
    for (n, p), q in zip(a.named_parameters(), t.parameters()):
        assert _same(p.detach(), q.detach()) and _same(p.grad, q.grad), n
        for k in ("exp_avg", "exp_avg_sq"):
            assert _same(oa.state[p][k], ot.state[q][k]), (n, k)


# ------------------------------------------------------------------------------------- tsr_adam_l2_step, the one-tensor form
def _f32(x):
    """x rounded to float, as a Python double: what a `float` argument of the C ABI receives."""
    return torch.tensor(x, dtype=torch.float32).item()


ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_WD = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(1e-8), _f32(1e-2)
ADAM_GUARD = 8


def _adam_state(n, step):
    g = torch.Generator().manual_seed(n % 1000 + step)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:        # a state as earlier steps leave it: sqrt(v) well above |m| / 50, so the update stays of the order of lr
        m, v = torch.randn(n, generator=g) * 1e-2, torch.rand(n, generator=g) * 1e-2 + 1e-3
    return p, gr, m, v


def _guarded(t):
    return torch.cat([t, torch.full((ADAM_GUARD,), float("nan"))]).cuda()


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("n", [1, 4095, 4097, 4096 * 256 + 7])
def test_adam_l2_step_one_tensor_form_vs_fp64_and_the_multi_form(n, step):
    """tsr_adam_l2_step (grid-stride, 4096 x 256 threads: n = 4096 * 256 + 7 takes a second trip) and tsr_adam_l2_multi
    on the same data cut into chunks of at most 4096, the multi form handed the float-rounded betas as doubles.

    The two are NOT bit-identical: they are the same formula, but the compiler fuses b1 * m + (1 - b1) * g' and
    b2 * v + ((1 - b2) g') g' into multiply-adds in the multi form's 16-byte path and leaves them as separate roundings
    in the one-tensor kernel (read off the gfx950 assembly), a legitimate last-bit difference.  Both are therefore held
    to fp64 Adam (the oracle's adam_l2_step) at the 1e-5 bar this file uses for the moments, per tensor, for the
    parameter and both moments.  (No tighter bar on the parameter: at step 1 the update lr * g' / (|g'| + eps') is
    ill-conditioned where g' = g + wd * w cancels to about eps, whatever the arithmetic.)"""
    import ctypes
    from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_float as Fl, c_longlong as L
    p, gr, m, v = _adam_state(n, step)
    ref = {"w": p.double()}
    state = {"w": {"m": m.double(), "v": v.double()}}
    O.adam_l2_step(ref, {"w": gr.double()}, state, step, ADAM_LR, ADAM_WD, (ADAM_B1, ADAM_B2), ADAM_EPS)
    want = dict(param=ref["w"], exp_avg=state["w"]["m"], exp_avg_sq=state["w"]["v"])

    one = [_guarded(t) for t in (p, gr, m, v)]
    call("tsr_adam_l2_step", *[ptr(t) for t in one], L(n), Fl(ADAM_LR), Fl(ADAM_B1), Fl(ADAM_B2), Fl(ADAM_EPS), Fl(ADAM_WD),
         I(step), stream())
    multi = [_guarded(t) for t in (p, gr, m, v)]
    recs = [tuple(t.data_ptr() + 4 * off for t in multi) + (min(optim.CHUNK, n - off), 0) for off in range(0, n, optim.CHUNK)]
    arr = (optim._Rec * len(recs))(*recs)
    table = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).clone().cuda()
    call("tsr_adam_l2_multi", ptr(table), I(len(recs)), Fl(ADAM_LR), ctypes.c_double(ADAM_B1), ctypes.c_double(ADAM_B2),
         Fl(ADAM_EPS), Fl(ADAM_WD), I(step), stream())
    torch.cuda.synchronize()
    for form, bufs in (("one-tensor", one), ("multi", multi)):
        got = dict(param=bufs[0].cpu(), exp_avg=bufs[2].cpu(), exp_avg_sq=bufs[3].cpu())
        assert torch.equal(bufs[1].cpu()[:n], gr), f"{form}: the gradient was written"
        for k, t in got.items():
            assert torch.isnan(t[n:]).all(), f"{form}: wrote behind {k}"
            err = float((t[:n].double() - want[k]).abs().max())
            rel = err / float(want[k].abs().max())
            print(f"[adam {form} n={n} step={step}] {k} {rel:.2e}")
            assert rel <= 1e-5, (form, k, rel)


@pytest.mark.parametrize("n,step", [(0, 1), (-5, 1), (16, 0), (16, -1)])
def test_adam_l2_step_rejects_empty_tensors_and_step_zero(n, step):
    from tactilesr_amd._lib import load, ptr, stream, c_int as I, c_float as Fl, c_longlong as L
    bufs = [torch.full((16,), float("nan"), device="cuda") for _ in range(4)]
    st = load().tsr_adam_l2_step(*[ptr(t) for t in bufs], L(n), Fl(ADAM_LR), Fl(ADAM_B1), Fl(ADAM_B2), Fl(ADAM_EPS), Fl(ADAM_WD),
                                 I(step), stream())
    torch.cuda.synchronize()
    assert st == 1 and all(torch.isnan(t).all() for t in bufs)
