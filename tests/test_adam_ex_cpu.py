"""CPU checks of the extended Adam launch (AdamW, AMSGrad): the restatement of tests/_adam_ex_cases.py IS torch's
AdamW / Adam(amsgrad) / AdamW(amsgrad) in fp64; tsr_adam_hyper_ex forms the floats its header defines; the three symbols
are declared, bound and exported under ABI 24; every refusal returns status 1 before any device call; state dicts go
both ways between tactilesr_amd.optim and torch.optim; decay_param_groups; fused_clip_applies; and optim.Adam without
amsgrad keeps the state keys and the row width it had."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _adam_ex_cases as AC
import tactilesr_amd
from tactilesr_amd import _lib, optim
from tactilesr_amd.optim import AdamW, decay_param_groups      # noqa: F401  (the feature: without it nothing here applies)
from tactilesr_amd.train import tactileSR_train as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsr_adam_hyper_ex", "tsr_adam_multi_ex", "tsr_adam_multi_ex_dev")
F, I, D, P = ctypes.c_float, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
NAN = float("nan")


def _torch_opt(flags, params, **kw):
    cls = torch.optim.AdamW if flags & AC.DECOUPLED else torch.optim.Adam
    return cls(params, amsgrad=bool(flags & AC.AMSGRAD), **kw)


def _our_opt(flags, params, **kw):
    cls = optim.AdamW if flags & AC.DECOUPLED else optim.Adam
    return cls(params, amsgrad=bool(flags & AC.AMSGRAD), **kw)


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("flags", [f for f, _ in AC.FLAG_CASES], ids=AC.FLAG_IDS)
def test_fp64_restatement_is_torchs_optimizer_over_five_steps_with_a_changing_lr(flags):
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 5, 3, 3), (33,), (1,), (4097,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64) * 0.1) for s in shapes]
    betas, eps, wd = (0.9, 0.999), 1e-8, 1e-2
    opt = _torch_opt(flags, params, lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    mine = [(p.detach().numpy().copy().ravel(), np.zeros(p.numel()), np.zeros(p.numel()), np.zeros(p.numel())) for p in params]
    worst = 0.0
    for it in range(5):
        lr = 1e-3 * (0.5 + it)
        opt.param_groups[0]["lr"] = lr
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** (it - 3) for s in shapes]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt.step()
        for k, (p, gr) in enumerate(zip(params, grads)):
            w, m, v, vm = mine[k]
            w, _, m, v, vm = AC.restate(w, gr.numpy().ravel(), m, v, vm, lr, betas, eps, wd, it + 1, flags)
            mine[k] = (w, m, v, vm if vm is not None else np.zeros_like(v))
            st = opt.state[p]
            pairs = [(w, p.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])]
            if flags & AC.AMSGRAD:
                pairs.append((vm, st["max_exp_avg_sq"]))
            for a, b in pairs:
                e = AC.relerr(a, b.numpy().ravel())
                worst = max(worst, e)
                assert e <= 1e-12, (it, k, e)
    print(f"[adam_ex restatement vs torch fp64] flags {flags}: worst {worst:.2e}")


def test_flags_zero_restatement_is_torch_adam():
    g = torch.Generator().manual_seed(6)
    p = torch.nn.Parameter(torch.randn(100, generator=g, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1e-3, weight_decay=1e-2)
    w, m, v = p.detach().numpy().copy(), np.zeros(100), np.zeros(100)
    for it in range(3):
        p.grad = torch.randn(100, generator=g, dtype=torch.float64)
        w, _, m, v, _ = AC.restate(w, p.grad.numpy(), m, v, None, 1e-3, (0.9, 0.999), 1e-8, 1e-2, it + 1, 0)
        opt.step()
        assert AC.relerr(w, p.detach().numpy()) <= 1e-12


def test_fp32_yardstick_stays_close_to_the_restatement():
    """The yardstick is the same formula: on a well-conditioned state it is within a few fp32 roundings of fp64."""
    p, g, m, v, vm = AC.state_case(5000, 3)
    for flags in AC.ALL_FLAGS:
        r64 = AC.restate(p, g, m, v, vm, AC.f32(1e-2), (0.9, 0.999), AC.f32(1e-8), AC.f32(0.1), 3, flags)
        r32 = AC.restate(p, g, m, v, vm, 1e-2, (0.9, 0.999), 1e-8, 0.1, 3, flags, dtype=np.float32)
        assert r32[0].dtype == np.float32 and AC.relerr(r32[0], r64[0]) < 5e-7, flags
        assert AC.relerr(r32[3], r64[3]) < 5e-7


# ------------------------------------------------------------------------------------------ tsr_adam_hyper_ex
@pytest.mark.parametrize("lr,b1,b2,step,wd", [(1e-3, 0.9, 0.999, 1, 1e-2), (1e-2, 0.9, 0.999, 7, 0.1),
                                              (3.7e-4, 0.5, 0.99, 1000, 0.0), (0.0, 0.0, 0.0, 1, 5.0),
                                              (1e-3 * 1e-4, 0.9, 0.999, 100000, 1e-2)])
def test_hyper_ex_is_the_legacy_floats_and_the_decay_as_defined(lr, b1, b2, step, wd):
    lib = _lib.load()
    o3 = (ctypes.c_float * 3)()
    assert lib.tsr_adam_hyper(F(lr), b1, b2, step, o3) == 0
    for flags in AC.ALL_FLAGS:
        o4 = (ctypes.c_float * 4)(NAN, NAN, NAN, NAN)
        assert lib.tsr_adam_hyper_ex(F(lr), b1, b2, step, F(wd), flags, o4) == 0
        got = np.array(list(o4), dtype=np.float32)
        assert AC.same_bits(got[:3], np.array(list(o3), dtype=np.float32)), flags
        want = np.float32(1.0 - float(np.float32(lr)) * float(np.float32(wd))) if flags & AC.DECOUPLED else np.float32(1.0)
        assert AC.same_bits(got[3:], np.array([want])), (flags, got[3], want)
        assert AC.same_bits(got, np.array(AC.hyper(lr, b1, b2, step, wd, flags), dtype=np.float32))


# ------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_bound_and_exported_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24
    for name, n_args in zip(NAMES, (7, 12, 11)):
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in include/tactilesr_hip.h"
        params = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        sig = _lib.SIGNATURES[name]
        assert len(params) == len(sig) == n_args, name
        assert [("*" in a) for a in params] == [t is ctypes.c_void_p for t in sig], name
        assert hasattr(lib, name)
    assert re.search(r"#define TSR_ADAM_DECOUPLED 1\b", header) and re.search(r"#define TSR_ADAM_AMSGRAD 2\b", header)
    assert (optim.DECOUPLED, optim.AMSGRAD) == (1, 2) == (AC.DECOUPLED, AC.AMSGRAD)
    src = os.path.join(REPO, "tactilesr_amd", "csrc", "adam_ex.hip")
    assert os.path.exists(src) and "tsr_adam_multi_ex" in open(src).read()
    # the legacy entry points keep their signatures
    assert len(_lib.SIGNATURES["tsr_adam_l2_multi"]) == 9 and len(_lib.SIGNATURES["tsr_adam_hyper"]) == 5


# ------------------------------------------------------------------------------------------ refusals
GOOD = dict(chunks=1, vmax=0, n_chunks=1, flags=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=1, hyper=1, out=1)
# every branch the header lists, as (reason, the arguments that differ from a good call)
REFUSALS = [
    ("chunks NULL", dict(chunks=0)), ("n_chunks = 0", dict(n_chunks=0)), ("n_chunks < 0", dict(n_chunks=-3)),
    ("an undefined flag bit", dict(flags=4)), ("an undefined flag bit beside a defined one", dict(flags=9)),
    ("negative flags", dict(flags=-1)),
    ("AMSGRAD without vmax", dict(flags=2)), ("AMSGRAD|DECOUPLED without vmax", dict(flags=3)),
    ("vmax without AMSGRAD (L2)", dict(flags=0, vmax=1)), ("vmax without AMSGRAD (DECOUPLED)", dict(flags=1, vmax=1)),
    ("eps NaN", dict(eps=NAN)), ("eps negative", dict(eps=-1e-8)),
    ("weight_decay NaN", dict(wd=NAN)), ("weight_decay negative", dict(wd=-1e-2)),
    ("beta1 = 1", dict(b1=1.0)), ("beta1 negative", dict(b1=-0.1)), ("beta1 NaN", dict(b1=NAN)),
    ("beta2 = 1", dict(b2=1.0)), ("beta2 negative", dict(b2=-0.1)), ("beta2 NaN", dict(b2=NAN)),
]
HOST_ONLY = [("step = 0", dict(step=0)), ("step < 0", dict(step=-2)), ("lr NaN", dict(lr=NAN)), ("lr negative", dict(lr=-1e-3))]
DEV_ONLY = [("hyper4 NULL", dict(hyper=0))]
HYPER_ONLY = [("out4 NULL", dict(out=0))]


def _call(form, **over):
    a = dict(GOOD, **over)
    lib = _lib.load()
    store = (ctypes.c_float * 64)()            # host memory: a refusal must return before anything looks at it
    addr = ctypes.addressof(store)
    p = lambda on: P(addr if on else 0)
    clip = P(0)
    if form == "host":
        return lib.tsr_adam_multi_ex(p(a["chunks"]), p(a["vmax"]), I(a["n_chunks"]), I(a["flags"]), F(a["lr"]), D(a["b1"]),
                                     D(a["b2"]), F(a["eps"]), F(a["wd"]), I(a["step"]), clip, P(0))
    if form == "dev":
        return lib.tsr_adam_multi_ex_dev(p(a["chunks"]), p(a["vmax"]), I(a["n_chunks"]), I(a["flags"]), p(a["hyper"]),
                                         D(a["b1"]), D(a["b2"]), F(a["eps"]), F(a["wd"]), clip, P(0))
    return lib.tsr_adam_hyper_ex(F(a["lr"]), D(a["b1"]), D(a["b2"]), I(a["step"]), F(a["wd"]), I(a["flags"]), p(a["out"]))


@pytest.mark.parametrize("reason,over", REFUSALS + HOST_ONLY, ids=[r for r, _ in REFUSALS + HOST_ONLY])
def test_host_scalar_form_refuses_before_any_device_call(reason, over):
    assert _call("host", **over) == 1, reason


@pytest.mark.parametrize("reason,over", REFUSALS + DEV_ONLY, ids=[r for r, _ in REFUSALS + DEV_ONLY])
def test_device_scalar_form_refuses_before_any_device_call(reason, over):
    assert _call("dev", **over) == 1, reason


# tsr_adam_hyper_ex takes no table, no eps and no hyper4, and flags 2 and 3 are good flags to it
HYPER_REFUSALS = [(r, o) for r, o in REFUSALS + HOST_ONLY + HYPER_ONLY
                  if not set(o) & {"chunks", "n_chunks", "vmax", "eps"} and o.get("flags") not in (2, 3)]


@pytest.mark.parametrize("reason,over", HYPER_REFUSALS, ids=[r for r, _ in HYPER_REFUSALS])
def test_hyper_ex_refuses(reason, over):
    assert _call("hyper", **over) == 1, reason


def test_hyper_refusal_table_covers_what_the_header_lists():
    reasons = {r for r, _ in HYPER_REFUSALS}
    for r in ("out4 NULL", "step = 0", "lr NaN", "lr negative", "weight_decay NaN", "weight_decay negative", "beta1 = 1",
              "beta2 NaN", "an undefined flag bit", "negative flags"):
        assert r in reasons, r
    assert _call("hyper") == 0        # the good call of the table is good


# ------------------------------------------------------------------------------------------ state dicts
def _stepped_torch(flags, seed=3, steps=3):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((4, 3), (5,))]
    opt = _torch_opt(flags, params, lr=1e-3, weight_decay=1e-2)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return params, opt


@pytest.mark.parametrize("flags", [f for f, _ in AC.FLAG_CASES], ids=AC.FLAG_IDS)
def test_state_dicts_round_trip_with_torchs_classes_both_ways(flags):
    params, topt = _stepped_torch(flags)
    sd = copy.deepcopy(topt.state_dict())      # load_state_dict keeps a tensor that needs no cast: no shared state
    mine = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ours = _our_opt(flags, mine, lr=5e-4, weight_decay=0.5)
    ours.load_state_dict(sd)                                        # torch -> ours
    keys = {"step", "exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if flags & AC.AMSGRAD else set())
    for p, q in zip(mine, params):
        assert set(ours.state[p]) == keys
        for k in keys:
            assert torch.equal(torch.as_tensor(ours.state[p][k]), torch.as_tensor(topt.state[q][k])), k
    assert ours.param_groups[0]["lr"] == 1e-3 and ours.param_groups[0]["weight_decay"] == 1e-2
    assert ours._flags(ours.param_groups[0]) == flags
    back = [torch.nn.Parameter(p.detach().clone()) for p in params]
    t2 = _torch_opt(flags, back, lr=7e-4, weight_decay=0.3)
    t2.load_state_dict(copy.deepcopy(ours.state_dict()))                        # ours -> torch
    g = torch.Generator().manual_seed(11)
    for p, q in zip(params, back):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    topt.step()
    t2.step()
    for p, q in zip(params, back):
        assert torch.equal(p, q)
        for k in keys:
            assert torch.equal(torch.as_tensor(topt.state[p][k]), torch.as_tensor(t2.state[q][k])), k


@pytest.mark.parametrize("cls", ["Adam", "AdamW"])
def test_loading_a_state_without_max_exp_avg_sq_into_amsgrad_raises(cls):
    params, topt = _stepped_torch(AC.DECOUPLED if cls == "AdamW" else 0)
    ours = getattr(optim, cls)([torch.nn.Parameter(p.detach().clone()) for p in params], amsgrad=True)
    with pytest.raises(KeyError, match="max_exp_avg_sq"):
        ours.load_state_dict(topt.state_dict())
    assert len(ours.state) == 0 and ours.param_groups[0]["amsgrad"] is True       # nothing was loaded
    # an empty state (an optimizer that never stepped) has nothing missing
    fresh = getattr(torch.optim, cls)([torch.nn.Parameter(p.detach().clone()) for p in params])
    ours.load_state_dict(fresh.state_dict())


# ------------------------------------------------------------------------------------------ decay_param_groups
def test_decay_param_groups_on_a_tactilesr():
    torch.manual_seed(0)
    m = tactilesr_amd.TactileSR(patternFeatureExtraLayerCnt=2)
    frozen = [p for n, p in m.named_parameters()][3:6]
    for p in frozen:
        p.requires_grad_(False)
    groups = optim.decay_param_groups(m, 1e-2)
    assert len(groups) == 2 and groups[0]["weight_decay"] == 0 and groups[1]["weight_decay"] == 1e-2
    assert "lr" not in groups[0] and "lr" not in groups[1]
    no_decay, decay = ({id(p) for p in g["params"]} for g in groups)
    everything = [id(p) for p in m.parameters()]
    listed = [id(p) for g in groups for p in g["params"]]
    assert sorted(listed) == sorted(everything) and len(set(listed)) == len(listed)      # none lost, none twice
    assert all(id(p) in no_decay | decay for p in frozen)                              # frozen parameters are kept
    n_bn = 0
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            for p in mod.parameters(recurse=False):
                n_bn += 1
                assert id(p) in no_decay
    assert n_bn > 0
    for p in m.parameters():
        if p.dim() <= 1:
            assert id(p) in no_decay
    assert decay and all(p.dim() > 1 for p in groups[1]["params"])
    order = {id(p): i for i, p in enumerate(m.parameters())}
    for g in groups:                                                                   # model.parameters() order
        idx = [order[id(p)] for p in g["params"]]
        assert idx == sorted(idx)
    with_lr = optim.decay_param_groups(m, 0.05, lr=3e-4)
    assert [g["lr"] for g in with_lr] == [3e-4, 3e-4] and with_lr[1]["weight_decay"] == 0.05
    opt = optim.AdamW(optim.decay_param_groups(m, 1e-2), lr=1e-3)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 1e-2] and [g["lr"] for g in opt.param_groups] == [1e-3] * 2


def test_fused_clip_applies_to_adamw_over_the_model_and_over_decay_param_groups():
    m = tactilesr_amd.TactileSR(patternFeatureExtraLayerCnt=2)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    assert isinstance(optim.AdamW(m.parameters()), optim.Adam)
    assert TR.fused_clip_applies(m, optim.AdamW(m.parameters(), lr=1e-3)) is True
    assert TR.fused_clip_applies(m, optim.AdamW(optim.decay_param_groups(m, 1e-2), lr=1e-3)) is True
    assert TR.fused_clip_applies(m, optim.Adam(optim.decay_param_groups(m, 1e-2), lr=1e-3, amsgrad=True)) is True
    assert TR.fused_clip_applies(m, torch.optim.AdamW(m.parameters())) is False
    assert TR.fused_clip_applies(m, optim.AdamW(list(m.parameters())[1:])) is False


# ------------------------------------------------------------------------------------------ the default path
def test_adam_without_amsgrad_keeps_its_state_keys_and_row_width(monkeypatch):
    # _replay_rows hands back PINNED rows, which needs a device; without one the same rows come from pageable memory
    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: empty(*a, **{**k, "pin_memory": False}))
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.Adam([p], lr=1e-3, weight_decay=1e-2)
    assert opt._flags(opt.param_groups[0]) == 0 and opt.hyper_width == 3 and opt.param_groups[0]["amsgrad"] is False
    st = {"step": torch.tensor(4.0), "exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3)}
    opt.state[p] = st
    rows = opt._replay_rows([(opt.param_groups[0], [st], None)])
    assert tuple(rows.shape) == (1, 3) and rows.stride() == (3, 1) and rows.dtype == torch.float32
    assert float(st["step"]) == 5 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
    o3 = (ctypes.c_float * 3)()
    assert _lib.load().tsr_adam_hyper(F(1e-3), 0.9, 0.999, 5, o3) == 0
    assert AC.same_bits(rows[0].numpy(), np.array(list(o3), dtype=np.float32))
    # the extended classes: four floats, formed by tsr_adam_hyper_ex
    for flags in (f for f, _ in AC.FLAG_CASES):
        q = torch.nn.Parameter(torch.zeros(3))
        o = _our_opt(flags, [q], lr=1e-2, weight_decay=0.1)
        s = {"step": torch.tensor(2.0), "exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "max_exp_avg_sq": torch.zeros(3)}
        rows = o._replay_rows([(o.param_groups[0], [s], None)])
        assert o.hyper_width == 4 and tuple(rows.shape) == (1, 4)
        assert AC.same_bits(rows[0].numpy(), np.array(AC.hyper(1e-2, 0.9, 0.999, 3, 0.1, flags), dtype=np.float32)), flags
    with pytest.raises(ValueError):
        optim.AdamW([p], weight_decay=-1.0)
    assert optim.AdamW([p]).defaults["weight_decay"] == 1e-2 and optim.Adam([p]).defaults["weight_decay"] == 0.0
