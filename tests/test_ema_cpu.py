"""Weight EMA / SWA without a GPU: the fp64 restatement and its derived bound, the decay schedules, the ABI bookkeeping
and the refusals of tsr_ema_multi / tsr_ema_multi_dev, WeightEMA's host logic on a CPU model (torch ops, same formula),
the checkpoint entry, recalibrate_bn's momentum sequence on a stub forward, and the ema=None defaults."""
import copy
import ctypes
import inspect
import os
import re

import pytest
import torch

import _ema_cases as EC
import tactilesr_amd
from tactilesr_amd import _lib
from tactilesr_amd.ema import WeightEMA, recalibrate_bn
from tactilesr_amd.train import checkpoint as CK
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Err = _lib.TactileSRHipError


# ------------------------------------------------------------------------------------------ restatement and bound
@pytest.mark.parametrize("omd", EC.OMDS)
def test_restatement_is_lerp_in_fp64(omd):
    for name, (avg, src) in EC.value_cases().items():
        want = torch.lerp(avg.double(), src.double(), EC.omd32(omd))
        got = EC.restatement(avg, src, omd)
        scale = torch.maximum(avg.double().abs(), src.double().abs()).clamp_min(1e-300)
        assert float(((got - want).abs() / scale).max()) <= 1e-15, name


@pytest.mark.parametrize("omd", EC.OMDS)
def test_bound_holds_for_the_fp32_evaluation(omd):
    for name, (avg, src) in EC.value_cases().items():
        got = EC.fp32_eval(avg, src, omd)
        worst = EC.check(got, avg, src, omd, label=f"{name} omd={omd}")
        print(f"[ema] fp32 evaluation, {name}, omd {omd}: worst {worst:.3f} of the bound")
    avg, src = EC.value_cases()["equal"]
    assert torch.equal(EC.bits(EC.fp32_eval(avg, src, omd)), EC.bits(avg))          # src == avg: unchanged bit for bit
    zero, src = EC.value_cases()["zero_avg"]
    if omd == 1.0:
        assert torch.equal(EC.bits(EC.fp32_eval(zero, src, omd)), EC.bits(src))     # avg == 0, omd == 1: src exactly


def test_the_checker_sees_a_wrong_result():
    avg, src = EC.value_cases()["normal"]
    got = EC.fp32_eval(avg, src, 0.5)
    got[17] = got[17] * (1 + 2.0 ** -20)
    with pytest.raises(AssertionError, match="outside"):
        EC.check(got, avg, src, 0.5)
    with pytest.raises(AssertionError):                       # decay and 1 - decay exchanged
        EC.check(EC.fp32_eval(avg, src, 1e-3), avg, src, 1 - 1e-3)


# ------------------------------------------------------------------------------------------ schedule
def _cpu_model(seed=3):
    torch.manual_seed(seed)
    return tactilesr_amd.TactileSR(10, 1, 3, 1, 1)


def test_decay_schedules():
    m = _cpu_model()
    e = WeightEMA(m, decay=0.999)
    assert [e.decay_at(t) for t in (0, 1, 1000)] == [0.999] * 3
    w = WeightEMA(m, decay=0.999, warmup=10)
    assert [w.decay_at(t) for t in range(3)] == [1 / 10, 2 / 11, 3 / 12]
    # (1 + t) / (10 + t) reaches 0.999 at t = 8990: below it before, saturated from there on
    assert w.decay_at(8989) == 8990 / 8999 < 0.999 and w.decay_at(8991) == 0.999 and w.decay_at(10 ** 6) == 0.999
    assert all(w.decay_at(t) <= w.decay_at(t + 1) for t in range(9100))
    s = WeightEMA(m, decay="swa")
    assert [s.decay_at(t) for t in range(4)] == [0.0, 1 / 2, 2 / 3, 3 / 4]
    # "swa" over x0..x4 in fp64 is their mean
    xs = torch.randn(5, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    avg = torch.full((64,), 123.0, dtype=torch.float64)      # whatever the shadow held: the first update replaces it
    for t in range(5):
        avg = avg + (1.0 - s.decay_at(t)) * (xs[t] - avg)
    # five updates of a few fp64 roundings each, every one relative to a value no larger than max |x|
    assert float((avg - xs.mean(0)).abs().max()) <= 16 * 2.0 ** -53 * float(xs.abs().max())
    assert w._omd(0) == float(1.0 - 0.1) and e._omd(5) == float(1.0 - 0.999)
    for bad in (dict(decay=1.5), dict(decay=-0.1), dict(decay="ema"), dict(warmup=0), dict(warmup=2.5),
                dict(decay="swa", warmup=3), dict(buffers="mean")):
        with pytest.raises(ValueError):
            WeightEMA(m, **bad)


# ------------------------------------------------------------------------------------------ ABI
def test_abi_symbols_declared_bound_exported():
    hdr = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    lib = _lib.load()
    for name in ("tsr_ema_multi", "tsr_ema_multi_dev"):
        assert re.search(rf"^int {name}\(const tsr_ema_chunk\* chunks, int n_chunks, int op, ", hdr, re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"typedef struct tsr_ema_chunk \{ float\* avg; float\* src; int n; int mode; \} tsr_ema_chunk;", hdr)
    assert _lib.SIGNATURES["tsr_ema_multi"] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    assert _lib.SIGNATURES["tsr_ema_multi_dev"] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_void_p]
    assert _lib.ABI_VERSION == 24 == lib.tsr_abi_version()
    assert ctypes.sizeof(EC.Rec) == 24 == ctypes.sizeof(tactilesr_amd.ema._Rec)


def test_refusals_return_status_1_before_any_device_call():
    """No GPU here: a refusal that reached the launch would not return 1 (no device: a launch failure, status 2)."""
    lib = _lib.load()
    table = (EC.Rec * 2)()                      # host memory: never dereferenced by a refused call
    t, scalar = ctypes.cast(table, ctypes.c_void_p), ctypes.cast((ctypes.c_float * 1)(0.5), ctypes.c_void_p)
    I, F, null = ctypes.c_int, ctypes.c_float, ctypes.c_void_p(0)
    bad_common = [(null, I(2), I(0)), (t, I(0), I(0)), (t, I(-3), I(0)), (t, I(2), I(-1)), (t, I(2), I(4))]
    for a in bad_common:
        assert lib.tsr_ema_multi(*a, F(0.5), null) == 1, a
        assert lib.tsr_ema_multi_dev(*a, scalar, null) == 1, a
    for omd in (float("nan"), -1e-6, 1.0 + 2.0 ** -20, float("inf"), -float("inf")):
        assert lib.tsr_ema_multi(t, I(2), I(0), F(omd), null) == 1, omd
    assert lib.tsr_ema_multi_dev(t, I(2), I(0), null, null) == 1


# ------------------------------------------------------------------------------------------ WeightEMA on a CPU model
def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
        for n, b in m.named_buffers():
            if b.dtype == torch.float32:
                b.add_(0.05 * torch.rand(b.shape, generator=g))
            else:
                b.add_(1)


def _snap(m):
    return {k: EC.bits(v) for k, v in m.state_dict().items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("buffers", ["copy", "ema"])
def test_cpu_model_shadow_and_three_updates(buffers):
    m = _cpu_model()
    e = WeightEMA(m, decay=0.999, warmup=10, buffers=buffers)
    sd = m.state_dict()
    assert list(e.shadow) == list(sd) and e.launches == 1 and e.updates == 0
    for k, v in sd.items():
        assert e.shadow[k].shape == v.shape and e.shadow[k].dtype == v.dtype and e.shadow[k].data_ptr() % 16 == 0
        assert torch.equal(EC.bits(e.shadow[k]), EC.bits(v))
    params = {n for n, _ in m.named_parameters()}
    for t in range(3):
        prev = {k: v.clone() for k, v in e.shadow.items()}
        _perturb(m, 10 + t)
        e.update()
        assert e.updates == t + 1 and e.launches == t + 2
        for k, v in m.state_dict().items():
            if v.dtype == torch.float32 and (k in params or buffers == "ema"):
                EC.check(e.shadow[k].reshape(-1), prev[k].reshape(-1), v.reshape(-1), 1.0 - e.decay_at(t), label=k)
                assert not torch.equal(e.shadow[k], v)
            else:                                   # copied: running statistics under "copy", num_batches_tracked always
                assert torch.equal(EC.bits(e.shadow[k]), EC.bits(v)), k
    nbt = [k for k in sd if k.endswith("num_batches_tracked")]
    assert nbt and all(int(e.shadow[k]) == 3 and e.shadow[k].dtype == torch.int64 for k in nbt)
    # the shadow loads into a fresh model
    fresh = _cpu_model(seed=9)
    fresh.load_state_dict(e.shadow)
    assert _same(_snap(fresh), {k: EC.bits(v) for k, v in e.shadow.items()})


def test_cpu_frozen_parameter_average_does_not_move():
    m = _cpu_model()
    e = WeightEMA(m, decay=0.9)
    frozen = next(iter(m.parameters()))
    before = EC.bits(frozen)
    with torch.no_grad():
        for p in list(m.parameters())[1:]:
            p.mul_(1.01)
    e.update()
    name = next(n for n, p in m.named_parameters() if p is frozen)
    assert torch.equal(EC.bits(e.shadow[name]), before)


def test_cpu_applied_swaps_and_restores_and_refuses_nested_calls():
    m = _cpu_model()
    e = WeightEMA(m, decay=0.5, buffers="ema")
    _perturb(m, 1)
    e.update()
    weights, shadow = _snap(m), {k: EC.bits(v) for k, v in e.shadow.items()}
    assert not _same(weights, shadow)
    ptrs = [t.data_ptr() for t in m.state_dict().values()]
    epoch = _lib.param_epoch()
    m._plan = "stale"
    with e.applied() as inside:
        assert inside is e and _same(_snap(m), shadow) and _same({k: EC.bits(v) for k, v in e.shadow.items()}, weights)
        assert m._plan is None and _lib.param_epoch() > epoch
        for call in (e.update, e.copy_to, e.reset, lambda: e.load_state_dict(e.state_dict())):
            with pytest.raises(Err, match="applied"):
                call()
        with pytest.raises(Err, match="applied"):
            with e.applied():
                pass
        epoch = _lib.param_epoch()
        m._plan = "stale"
    assert _same(_snap(m), weights) and _same({k: EC.bits(v) for k, v in e.shadow.items()}, shadow)
    assert m._plan is None and _lib.param_epoch() > epoch
    assert [t.data_ptr() for t in m.state_dict().values()] == ptrs          # addresses never change
    with pytest.raises(KeyError, match="boom"):
        with e.applied():
            raise KeyError("boom")
    assert _same(_snap(m), weights) and _same({k: EC.bits(v) for k, v in e.shadow.items()}, shadow)
    e.update()                                                              # usable again
    e.copy_to()
    assert _same(_snap(m), {k: EC.bits(v) for k, v in e.shadow.items()})
    other = _cpu_model(seed=5)
    e.copy_to(other)
    assert _same(_snap(other), _snap(m))
    e.reset()
    assert e.updates == 0


def test_cpu_state_dict_round_trip_and_mismatch():
    m = _cpu_model()
    e = WeightEMA(m, decay=0.99, warmup=4, buffers="ema")
    for t in range(2):
        _perturb(m, t)
        e.update()
    st = e.state_dict()
    assert set(st) == {"decay", "warmup", "buffers", "updates", "shadow"} and st["updates"] == 2
    assert all(v.data_ptr() != e.shadow[k].data_ptr() for k, v in st["shadow"].items())       # a copy, not the views
    f = WeightEMA(_cpu_model(seed=8))
    f.load_state_dict(st)
    assert (f.decay, f.warmup, f.buffers, f.updates) == (0.99, 4, "ema", 2)
    assert _same({k: EC.bits(v) for k, v in f.shadow.items()}, {k: EC.bits(v) for k, v in e.shadow.items()})
    k0 = next(iter(st["shadow"]))
    renamed = dict(st, shadow={("x." + k if k == k0 else k): v for k, v in st["shadow"].items()})
    with pytest.raises(Err, match="keys"):
        f.load_state_dict(renamed)
    reshaped = dict(st, shadow=dict(st["shadow"], **{k0: st["shadow"][k0].reshape(-1)[:-1].clone()}))
    with pytest.raises(Err, match=re.escape(k0)):
        f.load_state_dict(reshaped)
    # a model of other shapes is refused by copy_to, a reshaped tensor by update
    with pytest.raises(Err):
        e.copy_to(tactilesr_amd.TactileSR(10, 2, 3, 1, 1))
    p = next(iter(m.parameters()))
    p.data = torch.zeros(p.numel() + 1)
    with pytest.raises(Err, match="shadow holds"):
        e.update()


def test_cpu_moved_tensors_keep_the_shadow_and_mixed_devices_are_refused():
    m = _cpu_model()
    e = WeightEMA(m, decay=0.5)
    shadow_ptr = e._flat.data_ptr()
    for p in m.parameters():
        p.data = p.data.clone() + 1.0               # same names and shapes at new addresses
    prev = {k: v.clone() for k, v in e.shadow.items()}
    e.update()
    assert e._flat.data_ptr() == shadow_ptr
    for n, p in m.named_parameters():
        EC.check(e.shadow[n].reshape(-1), prev[n].reshape(-1), p.detach().reshape(-1), 0.5, label=n)
    # a replaced submodule is followed as well
    name, child = next((n, c) for n, c in m.named_children() if any(True for _ in c.parameters()))
    clone = copy.deepcopy(child)
    with torch.no_grad():
        for p in clone.parameters():
            p.add_(2.0)
    setattr(m, name, clone)
    prev = {k: v.clone() for k, v in e.shadow.items()}
    e.update()
    for n, p in m.named_parameters():
        EC.check(e.shadow[n].reshape(-1), prev[n].reshape(-1), p.detach().reshape(-1), 0.5, label=n)
    meta = _cpu_model()
    owner = next(c for c in meta.modules() if c._parameters)
    attr = next(iter(owner._parameters))
    setattr(owner, attr, torch.nn.Parameter(torch.empty(owner._parameters[attr].shape, device="meta")))
    with pytest.raises(Err, match="different devices"):
        WeightEMA(meta)


# ------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_with_and_without_ema(tmp_path):
    m = _cpu_model()
    e = WeightEMA(m, decay=0.9, warmup=3)
    _perturb(m, 4)
    e.update()
    path = str(tmp_path / "with.pth")
    CK.save_checkpoint(path, m, epoch=2, ema=e)
    m2 = _cpu_model(seed=12)
    e2 = WeightEMA(m2, decay=0.5)
    ck = CK.load_checkpoint(path, m2, epoch_len=10, ema=e2)         # the restricted unpickler suffices
    assert "ema_missing" not in ck and e2.updates == 1 and (e2.decay, e2.warmup) == (0.9, 3)
    assert _same({k: EC.bits(v) for k, v in e2.shadow.items()}, {k: EC.bits(v) for k, v in e.shadow.items()})
    assert _same(_snap(m2), _snap(m)) and not _same(_snap(m2), {k: EC.bits(v) for k, v in e2.shadow.items()})
    # a file saved without an EMA has exactly the key set it had before the option existed
    plain = str(tmp_path / "plain.pth")
    CK.save_checkpoint(plain, m, epoch=2)
    raw = torch.load(plain, map_location="cpu", weights_only=False)
    assert set(raw) == {"num_gpus", "model", "optimizer", "lr_scheduler", "metric_storage", "epoch"}
    assert set(torch.load(path, map_location="cpu", weights_only=False)) == set(raw) | {"ema"}
    e2.update()
    ck = CK.load_checkpoint(plain, m2, epoch_len=10, ema=e2)
    assert ck["ema_missing"] is True and e2.updates == 0
    assert _same({k: EC.bits(v) for k, v in e2.shadow.items()}, _snap(m2))            # reset from the loaded weights
    assert "ema_missing" not in CK.load_checkpoint(plain, m2, epoch_len=10)


# ------------------------------------------------------------------------------------------ recalibrate_bn
class _Stub(torch.nn.Module):
    """A stub forward on the CPU: torch's own BatchNorm in place of the train engine, which reads bn.momentum the same way."""

    def __init__(self):
        super().__init__()
        self.a, self.b, self.held = torch.nn.BatchNorm2d(3), torch.nn.BatchNorm2d(3), torch.nn.BatchNorm2d(3)
        self.b.momentum = 0.3
        self.seen = []

    def forward(self, x):
        self.seen.append((self.a.momentum, self.b.momentum, self.held.momentum, self.training, self.held.training,
                          torch.is_grad_enabled(), tuple(x.shape)))
        return self.held(self.b(self.a(x)))


def test_recalibrate_bn_momentum_sequence_and_restore():
    from tactilesr_amd.model.tactileSR_model import hold_bn_statistics
    m = _Stub().eval()
    hold_bn_statistics(m.held)
    m.train = lambda mode=True: (torch.nn.Module.train(m, mode), setattr(m.held, "training", False), m)[-1]
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randn(4, 5, 6, 6, generator=g) * (k + 1) + k, torch.zeros(4, 1, 60, 60)) for k in range(3)]
    weights = {n: p.detach().clone() for n, p in m.named_parameters()}
    held_before = (m.held.running_mean.clone(), m.held.running_var.clone(), int(m.held.num_batches_tracked))
    k = recalibrate_bn(m, batches, dict(seqsCnt=1, axisCnt=3))
    assert k == 3
    assert [s[:2] for s in m.seen] == [(1.0, 1.0), (1 / 2, 1 / 2), (1 / 3, 1 / 3)]
    assert all(s[2] == 0.1 and s[3] and not s[4] and not s[5] and s[6] == (4, 3, 6, 6) for s in m.seen)
    assert (m.a.momentum, m.b.momentum, m.held.momentum) == (0.1, 0.3, 0.1)          # restored
    assert not m.training and not m.a.training and not m.held.training              # the mode it came in
    x = [b[0][:, :3] for b in batches]
    mean = torch.stack([t.mean(dim=(0, 2, 3)) for t in x]).mean(0)
    var = torch.stack([t.var(dim=(0, 2, 3), unbiased=True) for t in x]).mean(0)
    assert torch.allclose(m.a.running_mean, mean, atol=1e-6) and torch.allclose(m.a.running_var, var, rtol=1e-5)
    assert int(m.a.num_batches_tracked) == 3 and int(m.held.num_batches_tracked) == held_before[2]
    assert torch.equal(m.held.running_mean, held_before[0]) and torch.equal(m.held.running_var, held_before[1])
    assert all(torch.equal(p.detach(), weights[n]) for n, p in m.named_parameters())
    # restored also when a forward raises, and a model that came in train mode leaves in train mode
    m.train()
    with pytest.raises(RuntimeError):
        recalibrate_bn(m, [torch.randn(4, 2, 6, 6)], dict(seqsCnt=1, axisCnt=3))       # 2 channels into BatchNorm2d(3)
    assert (m.a.momentum, m.b.momentum) == (0.1, 0.3) and m.training and m.a.training and not m.held.training


# ------------------------------------------------------------------------------------------ defaults
def test_ema_defaults_to_none_everywhere():
    for fn in (TR.train_one_iter, TR.eval_func, CK.save_checkpoint, CK.load_checkpoint, GraphedTrainStep.__init__):
        p = inspect.signature(fn).parameters
        assert "ema" in p and p["ema"].default is None, fn
    sig = inspect.signature(TR.train_one_iter)
    assert list(sig.parameters)[:4] == ["model", "optimizer", "batch", "config"]
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        grad_sync=None, check_finite=False, cur_iter=None, clip_grad_norm=0.0, ema=None)
    assert tactilesr_amd.WeightEMA is WeightEMA and tactilesr_amd.recalibrate_bn is recalibrate_bn
    p = inspect.signature(WeightEMA.__init__).parameters
    assert (p["decay"].default, p["warmup"].default, p["buffers"].default) == (0.999, None, "copy")
