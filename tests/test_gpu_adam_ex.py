"""The extended Adam launch on the device (tsr_adam_multi_ex / tsr_adam_multi_ex_dev: AdamW's decoupled weight decay,
AMSGrad) and tactilesr_amd.optim.AdamW / Adam(amsgrad=True) built on it.

  1. against torch        the legacy optimizer test's setup, for each of the three flag combinations
  2. boundaries           the size sweep and every pointer 1, 2, 3 floats off 16-byte alignment, against the restatement
  3. exact properties     bit for bit: pure decay, weight_decay = 0, the running maximum, the device-scalar form, the
                          clip form, skipped records
  4. non-finite values    a NaN and an Inf gradient element stay in their own element
  5. the step             train_one_iter, GraphedTrainStep, checkpoints, torch interoperability, the untouched default

The comparison rule, the restatement and the guarded harness (NaN-prefilled buffers between NaN guard bands, every
launch run twice from the same bits) are tests/_adam_ex_cases.py's.  Worst figures are printed next to their bars."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _adam_ex_cases as AC
import tactilesr_amd
from tactilesr_amd import _lib, optim
from tactilesr_amd.optim import AdamW, decay_param_groups      # noqa: F401  (the feature: without it nothing here applies)
from tactilesr_amd.ema import WeightEMA
from tactilesr_amd.train import checkpoint as CK
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep
from tactilesr_amd.train.lr_scheduler import LRWarmupScheduler

pytestmark = pytest.mark.gpu

FLAGS = [f for f, _ in AC.FLAG_CASES]
D, A = AC.DECOUPLED, AC.AMSGRAD
SCALARS = (AC.B_LR, AC.B_BETAS, AC.B_EPS, AC.B_WD)


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _cls(flags, torch_side=False):
    mod = torch.optim if torch_side else optim
    return mod.AdamW if flags & D else mod.Adam


def _tensor(n, seed, step=3):
    p, g, m, v, vm = AC.state_case(n, seed, step)
    return dict(param=p, grad=g, exp_avg=m, exp_avg_sq=v, vmax=vm)


def _same(x, y, names=None):
    return all(AC.same_bits(x[k], y[k]) for k in (names or x))


# ------------------------------------------------------------------------------------------ 1. against torch
@pytest.mark.parametrize("flags", FLAGS, ids=AC.FLAG_IDS)
def test_matches_torch_in_one_launch_per_step(flags):
    """The setup of test_gpu_train.py::test_fused_multi_tensor_adam_matches_torch_adam_in_one_launch_per_step: ragged
    sizes, a 4-byte-misaligned view, a parameter that never gets a gradient, five steps with a changing learning rate,
    gradient magnitudes from 1e-3 to 10; the parameter rule is that test's."""
    ams = bool(flags & A)
    g = torch.Generator().manual_seed(9)
    shapes = [(128, 128, 5, 5), (64, 256, 1, 1), (64,), (1, 128, 3, 3), (4097,), (3,), (5000,)]
    cpu = [torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in shapes]
    backing = torch.zeros(5001, device="cuda")
    dev = [torch.nn.Parameter(p.detach().clone().cuda()) for p in cpu[:-1]]
    odd = torch.nn.Parameter(backing[1:])                          # data_ptr % 16 == 4: scalar path
    with torch.no_grad():
        odd.copy_(cpu[-1])
    dev.append(odd)
    frozen_c, frozen_d = torch.nn.Parameter(torch.ones(7)), torch.nn.Parameter(torch.ones(7, device="cuda"))
    cpu64 = [torch.nn.Parameter(p.detach().double()) for p in cpu]
    kw = dict(lr=1e-3, weight_decay=1e-2, amsgrad=ams)
    ref64 = _cls(flags, True)(cpu64, **kw)
    ref = _cls(flags, True)(cpu + [frozen_c], **kw)
    opt = _cls(flags)(dev + [frozen_d], **kw)
    worst = (0.0, 0.0)
    for it in range(5):
        for pg in (ref.param_groups[0], opt.param_groups[0], ref64.param_groups[0]):
            pg["lr"] = 1e-3 * (0.5 + it)
        for pc, pd, p64 in zip(cpu, dev, cpu64):
            gr = torch.randn(pc.shape, generator=g) * (10.0 ** (it - 3))
            pc.grad, pd.grad, p64.grad = gr.clone(), gr.cuda(), gr.double()
        ref.step()
        ref64.step()
        opt.step()
        assert opt.launches == it + 1
        for pc, pd, p64 in zip(cpu, dev, cpu64):
            e_hip, e_ref = relerr(pd, p64), relerr(pc, p64)
            bar = max(1e-6, 4 * e_ref)
            print(f"[adam_ex vs torch] flags {flags} step {it + 1} {tuple(pc.shape)}: {e_hip:.2e} (bar {bar:.2e})")
            assert e_hip <= bar, (it, tuple(pc.shape), e_hip, e_ref)
            worst = max(worst, (e_hip, bar))
            keys = ("exp_avg_sq", "max_exp_avg_sq") if ams else ("exp_avg_sq",)
            for k in keys:
                e = relerr(opt.state[pd][k], ref.state[pc][k])
                assert e <= 1e-6, (it, k, tuple(pc.shape), e)
    print(f"[adam_ex vs torch] flags {flags}: worst parameter error {worst[0]:.2e} at a bar of {worst[1]:.2e}")
    assert torch.equal(frozen_d.cpu(), frozen_c.detach()) and len(opt.state[frozen_d]) == 0
    sd = opt.state_dict()
    want = {"step", "exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if ams else set())
    assert set(sd["state"][0]) == want and float(sd["state"][0]["step"]) == 5


# ------------------------------------------------------------------------------------------ 2. boundaries
BOUNDARY = [(f, oid, offs) for f in FLAGS for oid, offs in AC.offset_cases(f)]


@pytest.fixture(scope="module")
def sweep():
    return [_tensor(n, 100 + i) for i, n in enumerate(AC.SIZES)]


@pytest.mark.parametrize("flags,oid,offs", BOUNDARY, ids=[f"{dict(AC.FLAG_CASES)[f]}-{oid}" for f, oid, _ in BOUNDARY])
def test_sizes_and_misaligned_pointers(sweep, flags, oid, offs):
    got = AC.launch(sweep, flags, SCALARS, 3, offsets=offs)           # asserts the guards and the two runs itself
    worst = (0.0, 0.0)
    for t, o, n in zip(sweep, got, AC.SIZES):
        assert AC.same_bits(o["grad"], t["grad"])                       # no clipping: the gradient is only read
        worst = max(worst, AC.check_step(o, t, SCALARS, 3, flags, label=f"n = {n} {oid}"))
    print(f"[adam_ex boundaries] flags {flags} {oid}: worst parameter error {worst[0]:.2e} at a bar of {worst[1]:.2e}")


@pytest.mark.parametrize("flags", FLAGS, ids=AC.FLAG_IDS)
def test_first_step_from_a_zero_state(flags):
    tensors = [_tensor(n, 300 + n, step=1) for n in (5, 4097)]
    got = AC.launch(tensors, flags, SCALARS, 1)
    for t, o in zip(tensors, got):
        AC.check_step(o, t, SCALARS, 1, flags, label="step 1")


# ------------------------------------------------------------------------------------------ 3. exact properties
def test_pure_decay_is_one_rounded_multiply():
    """g = 0, m = v = 0: the Adam update is 0 / eps = 0, so p' is exactly fl32(p * decay)."""
    t = _tensor(4097 + 5, 1)
    z = np.zeros_like(t["param"])
    t.update(grad=z, exp_avg=z, exp_avg_sq=z, vmax=z)
    for flags in (D, D | A):
        got = AC.launch([t], flags, SCALARS, 4)[0]
        decay = AC.hyper(AC.B_LR, *AC.B_BETAS, 4, AC.B_WD, flags)[3]
        assert decay < 1 and AC.same_bits(got["param"], t["param"] * decay)
        assert not AC.same_bits(got["param"], t["param"])
        assert all(not got[k].any() for k in got if k != "param")


def test_zero_weight_decay_makes_both_forms_the_same_bits():
    tensors = [_tensor(n, 7 + n) for n in (3, 1025, 4096 + 9)]
    sc = (AC.B_LR, AC.B_BETAS, AC.B_EPS, 0.0)
    for ams in (0, A):
        l2 = AC.launch(tensors, ams, sc, 3)
        dec = AC.launch(tensors, ams | D, sc, 3)
        assert all(_same(x, y) for x, y in zip(l2, dec)), ams
        assert not AC.same_bits(l2[1]["param"], tensors[1]["param"])
    # ... and a weight decay does tell them apart
    assert not AC.same_bits(AC.launch(tensors, 0, SCALARS, 3)[1]["param"], AC.launch(tensors, D, SCALARS, 3)[1]["param"])


@pytest.mark.parametrize("flags", [A, D | A], ids=["adam_amsgrad", "adamw_amsgrad"])
def test_running_maximum_is_torch_maximum_of_the_launchs_own_v(flags):
    tensors = [_tensor(n, 17 + n) for n in (67, 4099)]
    got = AC.launch(tensors, flags, SCALARS, 3)
    for t, o in zip(tensors, got):
        want = torch.maximum(torch.from_numpy(t["vmax"]), torch.from_numpy(o["exp_avg_sq"])).numpy()
        assert AC.same_bits(o["vmax"], want)
        rose = o["exp_avg_sq"] > t["vmax"]
        assert rose.any() and (~rose).any()                              # both sides of the maximum were exercised
    # without AMSGRAD the same step divides by v itself: another parameter
    plain = AC.launch(tensors, flags & D, SCALARS, 3)
    assert not AC.same_bits(plain[1]["param"], got[1]["param"]) and AC.same_bits(plain[1]["exp_avg_sq"], got[1]["exp_avg_sq"])


@pytest.mark.parametrize("coef", [None, 0.25], ids=["plain", "clip"])
@pytest.mark.parametrize("flags", AC.ALL_FLAGS, ids=["adam"] + AC.FLAG_IDS)
def test_device_scalar_form_is_the_host_scalar_form(flags, coef):
    tensors = [_tensor(n, 27 + n) for n in (5, 4096 + 11)]
    host = AC.launch(tensors, flags, SCALARS, 6, coef=coef)
    dev = AC.launch(tensors, flags, SCALARS, 6, coef=coef, dev_form=True)
    assert all(_same(x, y) for x, y in zip(host, dev))
    # the device form reads hyper4, not the arguments it is handed beside it: another row, another result
    other = AC.launch(tensors, flags, SCALARS, 6, coef=coef, dev_form=True,
                      hyper4=AC.hyper(2 * AC.B_LR, *AC.B_BETAS, 6, AC.B_WD, flags))
    assert not AC.same_bits(other[1]["param"], host[1]["param"])


@pytest.mark.parametrize("coef", [1.0, 0.25])
@pytest.mark.parametrize("flags", AC.ALL_FLAGS, ids=["adam"] + AC.FLAG_IDS)
def test_clip_form_is_the_multiply_then_the_unclipped_launch(flags, coef):
    tensors = [_tensor(n, 37 + n) for n in (7, 4096 + 13)]
    for offs in ({}, {"grad": 1}):                                       # the vector and the scalar path
        clipped = AC.launch(tensors, flags, SCALARS, 3, coef=coef, offsets=offs)
        pre = [dict(t, grad=(t["grad"] * np.float32(coef)).astype(np.float32)) for t in tensors]
        plain = AC.launch(pre, flags, SCALARS, 3, offsets=offs)
        assert all(_same(x, y) for x, y in zip(clipped, plain)), offs
        for t, o in zip(tensors, clipped):
            assert AC.same_bits(o["grad"], t["grad"]) == (coef == 1.0)   # left clipped in place; untouched at 1
            AC.check_step(o, t, SCALARS, 3, flags, coef=coef, label=f"clip {coef}")


@pytest.mark.parametrize("bad_n", [0, 4097, -1])
@pytest.mark.parametrize("flags", AC.ALL_FLAGS, ids=["adam"] + AC.FLAG_IDS)
def test_a_record_with_n_outside_1_4096_is_skipped(flags, bad_n):
    tensors = [_tensor(n, 47 + n) for n in (300, 5000, 300)]
    got = AC.launch(tensors, flags, SCALARS, 3, override={1: (bad_n,)}, coef=0.5)
    names = [k for k in got[1]]
    assert _same(got[1], tensors[1], names)                              # nothing written through its pointers
    for i in (0, 2):
        assert not AC.same_bits(got[i]["param"], tensors[i]["param"])
        AC.check_step(got[i], tensors[i], SCALARS, 3, flags, coef=0.5, label="neighbour of a bad record")


# ------------------------------------------------------------------------------------------ 4. non-finite values
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("flags", FLAGS, ids=AC.FLAG_IDS)
def test_a_non_finite_gradient_element_stays_in_its_own_element(flags, bad):
    n = 4096 + 300
    t = _tensor(n, 57)
    spots = (5, 4096 + 257)                                              # a vector lane and a scalar tail word
    dirty = dict(t, grad=t["grad"].copy())
    dirty["grad"][list(spots)] = bad
    clean = AC.launch([t], flags, SCALARS, 3)[0]
    got = AC.launch([dirty], flags, SCALARS, 3)[0]
    keep = np.ones(n, bool)
    keep[list(spots)] = False
    want = AC.restate(dirty["param"], dirty["grad"], t["exp_avg"], t["exp_avg_sq"], t["vmax"], *SCALARS, 3, flags,
                      dtype=np.float32)
    names = ["param", "exp_avg", "exp_avg_sq"] + (["vmax"] if flags & A else [])
    for k, w in zip(names, [want[0], want[2], want[3], want[4]]):
        assert AC.same_bits(got[k][keep], clean[k][keep]), k             # every other element: the run without them
        for s in spots:
            if np.isnan(w[s]):
                assert np.isnan(got[k][s]), (k, s)
            else:
                assert got[k][s] == w[s], (k, s, got[k][s], w[s])
    for s in spots:
        if np.isnan(bad):                                                # the NaN is in p, m, v and vmax
            assert all(np.isnan(got[k][s]) for k in names)
        else:                                                            # Inf: m, v (vmax) Inf, the step Inf / Inf = NaN
            assert np.isinf(got["exp_avg"][s]) and np.isinf(got["exp_avg_sq"][s]) and np.isnan(got["param"][s])
            assert not flags & A or np.isinf(got["vmax"][s])


# ------------------------------------------------------------------------------------------ 5. the step
CFG = dict(patternFeatureExtraLayerCnt=2)
CONF = TR.default_config()
CLIP = 0.05


def _model(seed=42):
    torch.manual_seed(seed)
    return tactilesr_amd.TactileSR(**CFG).cuda().train()


def _batches(n, seed=7, B=4):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (torch.rand(B, 1, 100, 100, generator=g) * 250).cuda())
            for _ in range(n)]


def _adamw(m, amsgrad=False):
    return optim.AdamW(optim.decay_param_groups(m, 1e-2), lr=1e-3, amsgrad=amsgrad)


def _sched(opt):
    return LRWarmupScheduler(torch.optim.lr_scheduler.StepLR(opt, 2, 0.8), epoch_len=4, warmup_t=8, warmup_mode="auto",
                             warmup_factor=1e-4)


def _tick(sched, i):
    sched.iter_update()
    if (i + 1) % 4 == 0:
        sched.epoch_update()


STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _snap(m, opt, ema=None):
    out = {k: AC.bits(v) for k, v in m.state_dict().items()}
    for i, p in enumerate(m.parameters()):
        st = opt.state[p]
        out[f"opt.{i}.step"] = AC.bits(st["step"].float())
        out.update({f"opt.{i}.{k}": AC.bits(st[k]) for k in STATE_KEYS if k in st})
    if ema is not None:
        out.update({f"ema.{k}": AC.bits(v) for k, v in ema.shadow.items()})
    return out


def _assert_same(a, b, what=""):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k}"


def _np(t):
    return t.detach().cpu().numpy().ravel().copy()


@pytest.mark.parametrize("amsgrad", [False, True], ids=["adamw", "adamw_amsgrad"])
def test_three_clipped_steps_follow_the_restatement_on_the_devices_own_gradients(amsgrad):
    m = _model()
    opt = _adamw(m, amsgrad)
    sched = _sched(opt)
    flags = D | (A if amsgrad else 0)
    group_of = {id(p): g for g in opt.param_groups for p in g["params"]}
    names = {id(p): n for n, p in m.named_parameters()}
    worst, acted = (0.0, 0.0), 0
    for t, batch in enumerate(_batches(3)):
        before = {}
        for p in m.parameters():
            st = opt.state[p]
            z = np.zeros(p.numel(), np.float32)
            before[id(p)] = dict(param=_np(p), exp_avg=_np(st["exp_avg"]) if st else z, exp_avg_sq=_np(st["exp_avg_sq"]) if st else z,
                                 vmax=_np(st["max_exp_avg_sq"]) if st and amsgrad else z)
        launches = opt.launches
        TR.train_one_iter(m, opt, batch, CONF, clip_grad_norm=CLIP)
        assert opt.launches - launches == optim.GN_LAUNCHES + 2           # the fused path: the norm, then one per group
        norm = float(torch.nn.utils.get_total_norm([p.grad for p in m.parameters()]))
        acted += norm >= CLIP * (1 - 1e-4)
        assert norm <= CLIP * (1 + 1e-4)
        for p in m.parameters():
            g = group_of[id(p)]
            st = opt.state[p]
            assert float(st["step"]) == t + 1
            # the launch left the clipped gradient in p.grad: the restatement takes the step on exactly that
            b = dict(before[id(p)], grad=_np(p.grad))
            got = dict(param=_np(p), grad=_np(p.grad), exp_avg=_np(st["exp_avg"]), exp_avg_sq=_np(st["exp_avg_sq"]))
            if amsgrad:
                got["vmax"] = _np(st["max_exp_avg_sq"])
            sc = (g["lr"], g["betas"], g["eps"], g["weight_decay"])
            worst = max(worst, AC.check_step(got, b, sc, t + 1, flags, label=f"step {t + 1} {names[id(p)]}"))
        _tick(sched, t)
    assert acted == 3, "clip_grad_norm = 0.05 was meant to act on every step"
    assert len({g["lr"] for g in opt.param_groups}) == 1 and opt.param_groups[0]["weight_decay"] == 0
    print(f"[adam_ex step] amsgrad={amsgrad}: worst parameter error {worst[0]:.2e} at a bar of {worst[1]:.2e}")


@pytest.mark.parametrize("amsgrad", [False, True], ids=["adamw", "adamw_amsgrad"])
def test_graphed_step_matches_eager_bit_for_bit_with_clipping_and_a_warming_ema(amsgrad):
    batches = _batches(4, seed=13)
    me, mg = _model(), _model()
    oe, og = _adamw(me, amsgrad), _adamw(mg, amsgrad)
    se, sg = _sched(oe), _sched(og)
    ee, eg = WeightEMA(me, decay=0.999, warmup=10), WeightEMA(mg, decay=0.999, warmup=10)
    gstep = GraphedTrainStep(mg, og, CONF, warmup=1, clip_grad_norm=CLIP, ema=eg)
    lrs = []
    for t, b in enumerate(batches):                                      # one eager call + three replays
        le = TR.train_one_iter(me, oe, b, CONF, clip_grad_norm=CLIP, ema=ee)["total_loss"].detach().clone()
        lg = gstep(b)["total_loss"].detach().clone()
        lrs.append(og.param_groups[1]["lr"])
        assert torch.equal(le, lg), t
        _assert_same(_snap(me, oe, ee), _snap(mg, og, eg), f"step {t}")
        _tick(se, t)
        _tick(sg, t)
    assert gstep.captures == 1 and len(set(lrs)) == 4
    assert oe.launches == og.launches == 4 * (optim.GN_LAUNCHES + 2)
    assert tuple(gstep._hyper.shape)[1] == 4 == og.hyper_width
    assert ("max_exp_avg_sq" in og.state[next(mg.parameters())]) == amsgrad


def test_legacy_adam_graph_keeps_three_float_rows():
    m = _model()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    gstep = GraphedTrainStep(m, opt, CONF, warmup=1)
    for b in _batches(2):
        gstep(b)
    assert gstep.captures == 1 and tuple(gstep._hyper.shape)[1] == 3 and gstep._hyper.stride() == (3, 1)


def test_amsgrad_checkpoint_round_trip_continues_bit_identically(tmp_path):
    batches = _batches(4, seed=17)
    m = _model()
    opt = _adamw(m, amsgrad=True)
    for b in batches[:2]:
        TR.train_one_iter(m, opt, b, CONF, clip_grad_norm=CLIP)
    path = str(tmp_path / "amsgrad.pth")
    CK.save_checkpoint(path, m, opt, iteration=2)
    m2 = _model(seed=9)
    opt2 = _adamw(m2, amsgrad=True)
    CK.load_checkpoint(path, m2, opt2)
    assert all(opt2.state[p]["max_exp_avg_sq"].is_cuda for p in m2.parameters())
    _assert_same(_snap(m, opt), _snap(m2, opt2), "after loading")
    for b in batches[2:]:
        TR.train_one_iter(m, opt, b, CONF, clip_grad_norm=CLIP)
        TR.train_one_iter(m2, opt2, b, CONF, clip_grad_norm=CLIP)
    _assert_same(_snap(m, opt), _snap(m2, opt2), "two steps after loading")
    assert float(opt2.state[next(m2.parameters())]["step"]) == 4
    # a checkpoint written without AMSGrad is refused by an amsgrad=True optimizer
    m3 = _model()
    o3 = _adamw(m3)
    TR.train_one_iter(m3, o3, batches[0], CONF)
    CK.save_checkpoint(path, m3, o3, iteration=1)
    with pytest.raises(KeyError, match="max_exp_avg_sq"):
        CK.load_checkpoint(path, _model(), opt2)


@pytest.mark.parametrize("amsgrad", [False, True], ids=["adamw", "adamw_amsgrad"])
def test_torch_adamw_loads_our_state_and_one_further_step_agrees(amsgrad):
    batches = _batches(3, seed=19)
    m = _model()
    opt = _adamw(m, amsgrad)
    for b in batches[:2]:
        TR.train_one_iter(m, opt, b, CONF)
    twins = []
    for dtype in (torch.float32, torch.float64):
        c = tactilesr_amd.TactileSR(**CFG)
        c.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        c = c.to(dtype)
        topt = torch.optim.AdamW(optim.decay_param_groups(c, 1e-2), lr=1e-3, amsgrad=amsgrad)
        topt.load_state_dict(copy.deepcopy(opt.state_dict()))
        p0 = next(c.parameters())
        assert topt.state[p0]["exp_avg"].dtype == dtype and not topt.state[p0]["exp_avg"].is_cuda
        assert float(topt.state[p0]["step"]) == 2
        twins.append((c, topt))
    # the device's own gradients of a third batch, handed to all three
    for p in m.parameters():
        p.grad = None
    loss, _ = TR.train_cal_loss(m, batches[2], CONF)
    loss.backward()
    for c, topt in twins:
        for p, q in zip(m.parameters(), c.parameters()):
            q.grad = p.grad.detach().cpu().to(q.dtype)
        topt.step()
    opt.step()
    (c32, _), (c64, _) = twins
    worst = (0.0, 0.0)
    for (n, p), q32, q64 in zip(m.named_parameters(), c32.parameters(), c64.parameters()):
        e_hip, e_ref = relerr(p, q64), relerr(q32, q64)
        bar = max(1e-6, 4 * e_ref)
        assert e_hip <= bar, (n, e_hip, e_ref)
        worst = max(worst, (e_hip, bar))
    print(f"[adam_ex torch interop] amsgrad={amsgrad}: worst parameter error {worst[0]:.2e} at a bar of {worst[1]:.2e}")


def test_grad_sync_steps_with_adamw_from_the_arena():
    """GradSync on a single-rank RCCL group (the mean over one rank is the identity): the clipped AdamW + AMSGrad steps
    equal the un-synced ones bit for bit, and the chunk tables (two groups and the norm's) are built once."""
    import os
    import socket
    import torch.distributed as dist
    from tactilesr_amd import ddp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    ddp.init_distributed("nccl")
    try:
        batches = _batches(3, seed=29)
        m, r = _model(), _model()
        om, orr = _adamw(m, amsgrad=True), _adamw(r, amsgrad=True)
        sync = ddp.GradSync(m)
        assert sync.world == 1
        for b in batches:
            TR.train_one_iter(m, om, b, CONF, grad_sync=sync, clip_grad_norm=CLIP)
            TR.train_one_iter(r, orr, b, CONF, clip_grad_norm=CLIP)
        _assert_same(_snap(m, om), _snap(r, orr), "with and without GradSync")
        assert om.launches == 3 * (optim.GN_LAUNCHES + 2) and om.table_builds == 3
    finally:
        dist.destroy_process_group()


def test_adam_without_amsgrad_still_issues_tsr_adam_l2_multi():
    """The default path was not rerouted: one optim.Adam step equals tsr_adam_l2_multi applied by hand, bit for bit."""
    m = _model()
    loss, _ = TR.train_cal_loss(m, _batches(1, seed=23)[0], CONF)
    loss.backward()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    params = list(m.parameters())
    hand = [(p.detach().clone(), p.grad.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    recs = []
    for tensors in hand:
        n = tensors[0].numel()
        recs += [tuple(t.data_ptr() + 4 * off for t in tensors) + (min(optim.CHUNK, n - off), 0) for off in range(0, n, optim.CHUNK)]
    arr = (optim._Rec * len(recs))(*recs)
    table = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).clone().cuda()
    _lib.call("tsr_adam_l2_multi", _lib.ptr(table), ctypes.c_int(len(recs)), ctypes.c_float(1e-3), ctypes.c_double(0.9),
              ctypes.c_double(0.999), ctypes.c_float(1e-8), ctypes.c_float(1e-2), ctypes.c_int(1), _lib.stream())
    opt.step()
    assert opt.launches == 1 and opt.hyper_width == 3
    for (n, p), (hp, hg, hm, hv) in zip(m.named_parameters(), hand):
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}, n
        assert torch.equal(AC.bits(p), AC.bits(hp)) and torch.equal(AC.bits(p.grad), AC.bits(hg)), n
        assert torch.equal(AC.bits(st["exp_avg"]), AC.bits(hm)) and torch.equal(AC.bits(st["exp_avg_sq"]), AC.bits(hv)), n
