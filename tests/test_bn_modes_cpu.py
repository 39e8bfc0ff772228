"""Host-side tests of eval-mode BatchNorm layers inside the train step: the per-layer-mode fp64 reference (tests/_bn_modes.py)
pinned against the oracle, the backward plan with held layers, the four entry points' declaration and refusals,
``hold_bn_statistics`` / ``model_param_init(hold_bn=True)``, and the engines' control flow without a device."""
import ctypes
import inspect
import os
import re
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O
from tactilesr_amd.model._train import backward_plan, block_backward_plan, bn_held

import _bn_modes as BM
import _frozen as FZ
import _gradcheck as GC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(scale_factor=3, seqsCnt=2, patternFeatureExtraLayerCnt=2, forceFeatureExtraLayerCnt=1)
ENTRY_POINTS = ("tsr_bn_eval_vectors", "tsr_bn_bwd_finalize_eval", "tsr_bn_bwd_apply_eval", "tsr_bn_bwd_apply_eval_b16")


def _cpu_model(seed=5, **over):
    import tactilesr_amd
    cfg = dict(CFG, **over)
    sd, LR, HR = GC.step_data(cfg, 3, seed)
    m = tactilesr_amd.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    return m, sd, LR, HR


# --------------------------------------------------------------------------------------- the reference helper vs the oracle
def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("held", [False, True])
def test_helper_equals_the_oracle_where_the_oracle_can_speak(held):
    """All layers training / all layers held are the oracle's `training=True` / `training=False`: outputs, every parameter
    gradient and the new running statistics agree to 1e-10 relative (both sides are fp64 torch on the same ops; the bound
    only allows for summation order)."""
    m, sd, LR, HR = _cpu_model()
    BM.set_modes(m, BM.bn_paths(m) if held else [])
    dt = torch.float64
    leaves = {k: v.detach().to(dt).requires_grad_(True) for k, v in sd.items() if O.is_trainable(k)}
    full = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    full.update(leaves)
    ns_o = {}
    tap = O.ReluTap(record=True)
    out_o = O.tactilesr_forward(full, LR.to(dt), scale_factor=CFG["scale_factor"], training=not held, new_stats=ns_o, tap=tap)
    g_o = dict(zip(leaves, torch.autograd.grad(F.mse_loss(out_o, HR.to(dt)), list(leaves.values()))))
    out_h = BM.forward(m, LR)
    assert _rel(out_h, out_o.detach()) < 1e-10
    loss, g_h, ns_h, pre, _ = BM.step(m, LR, HR, record=True)
    assert abs(loss - float(F.mse_loss(out_o, HR.to(dt)).detach())) < 1e-10 * abs(loss)
    assert set(g_h) == set(g_o)
    scale = max(float(v.abs().max()) for v in g_o.values())
    for k, ref in g_o.items():
        if float(ref.abs().max()) < 1e-9 * scale:          # conv bias in front of a train-mode BatchNorm: 0 + noise on both sides
            assert float(g_h[k].abs().max()) < 1e-9 * scale, k
            continue
        assert _rel(g_h[k], ref) < 1e-10, k
    assert set(pre) == set(tap.pre)
    if held:
        assert ns_h == {} and ns_o == {}
        # with held statistics the conv biases in front of the BatchNorm layers get real gradients
        assert float(g_h["patternFeatureExtra_layer.0.conv_3_1.0.bias"].abs().max()) > 1e-6 * scale
    else:
        assert set(ns_h) == set(ns_o)
        for k, v in ns_o.items():
            assert _rel(ns_h[k], v) < 1e-10 if v.is_floating_point() else int(ns_h[k]) == int(v), k


def test_helper_honours_each_layers_own_flag():
    """Mixed modes: a held layer is absent from the new statistics, a training one present; the output differs from both
    uniform modes."""
    m, sd, LR, HR = _cpu_model()
    held = BM.pattern_paths(m, "mixed")
    BM.set_modes(m, held)
    ns = {}
    out = BM.forward(m, LR, new_stats=ns)
    assert {k.rsplit(".", 1)[0] for k in ns} == set(BM.bn_paths(m)) - set(held)
    o_train = BM.forward(BM.set_modes(m, []), LR)
    o_eval = BM.forward(BM.set_modes(m, BM.bn_paths(m)), LR)
    assert _rel(out, o_train) > 1e-6 and _rel(out, o_eval) > 1e-6
    assert len(BM.bn_paths(m)) == 2 * 2 + 1 + 4 * 2 and len(BM.trunk_bn_paths(m)) == 8


# -------------------------------------------------------------------------------------------------------------- the plan
def _seqs_plan(T=2, M=3):
    names = FZ.param_names(T, M, 1)
    trunk_bn = frozenset(f"patternFeatureExtra_layer.{i}.{c}.1" for i in range(M) for c in FZ.MSRB_CONVS)
    want = frozenset(n for n in names if not FZ.is_trunk(n))
    return names, trunk_bn, want


def test_plan_of_the_seqs_case_has_one_scale_pass_per_trunk_batchnorm_and_nothing_else_for_it():
    names, trunk_bn, want = _seqs_plan()
    plan = backward_plan(2, 3, 1, want, False, bn_eval=trunk_bn)
    trunk = [r for r in plan if r.layer.startswith("patternFeatureExtra_layer.")]
    assert not [r for r in trunk if r.kind == "bn_bwd_finalize"]
    applies = [r for r in trunk if r.kind == "bn_bwd_apply"]
    assert len(applies) == 3 * 3                                     # per MSRB: conv_3_2.1, conv_5_2.1, the stage-1 pair
    assert all(not any(t.endswith(".coef") for t in r.consumes) and len(r.consumes) == 1 for r in applies)
    for i, r in enumerate(plan):
        if r.kind == "bn_bwd_apply" and r in trunk:
            prod = [q for q in plan[:i] if r.consumes[0] in q.produces]
            assert len(prod) == 1 and prod[0].kind == "dgrad"
            assert not any(t.endswith(".sums") for t in prod[0].produces), prod[0]
    # the non-trunk BatchNorm layers keep today's records (inputContact_layer.1 gets its sums from the first MSRB's last dgrad)
    last = [r for r in plan if r.key == ("dgrad", "patternFeatureExtra_layer.0.conv_5_1.0")][0]
    assert last.produces == ("patternFeatureExtra_layer.0.dx", "patternFeatureExtra_layer.0.dx.sums")
    assert ("bn_bwd_finalize", "inputContact_layer.1") in {r.key for r in plan}
    # against the same want-set with batch statistics: 9 finalize records fewer, everything else launch for launch
    base = backward_plan(2, 3, 1, want, False)
    assert [r.key for r in plan] == [r.key for r in base if not (r.kind == "bn_bwd_finalize" and r.layer.startswith("patternFeature"))]


@pytest.mark.parametrize("T,M,R,dx", [(1, 2, 1, False), (2, 3, 2, True)])
def test_plan_with_no_held_layer_is_todays_plan_record_for_record(T, M, R, dx):
    names = FZ.param_names(T, M, R)
    for pat in FZ.PATTERNS:
        want, wdx = FZ.PATTERNS[pat](names)
        assert backward_plan(T, M, R, want, wdx or dx, bn_eval=frozenset()) == backward_plan(T, M, R, want, wdx or dx)
    assert block_backward_plan("msrb", frozenset(FZ.msrb_names()), True, bn_eval=frozenset()) == \
        block_backward_plan("msrb", frozenset(FZ.msrb_names()), True)
    assert "bn_eval" in inspect.signature(backward_plan).parameters and "bn_eval" in inspect.signature(block_backward_plan).parameters
    assert inspect.signature(backward_plan).parameters["bn_eval"].default == frozenset()


def test_held_layer_with_a_wanted_gamma_keeps_its_finalize_and_the_sums():
    names, trunk_bn, want = _seqs_plan()
    bn = "patternFeatureExtra_layer.1.conv_5_2.1"
    plan = backward_plan(2, 3, 1, want | {bn + ".weight"}, False, bn_eval=trunk_bn)
    fin = [r for r in plan if r.kind == "bn_bwd_finalize" and r.layer.startswith("patternFeature")]
    assert [r.layer for r in fin] == [bn] and fin[0].produces == ()
    dg = [r for r in plan if r.key == ("dgrad", "patternFeatureExtra_layer.1.confusion[128:256]")][0]
    assert dg.produces[1].endswith(".sums")
    ap = [r for r in plan if r.key == ("bn_bwd_apply", bn)][0]
    assert ap.consumes == (dg.produces[0],)


def test_mixed_stage_one_pair_keeps_the_batch_statistics_records():
    """The two stage-1 layers share their backward launches: held only when both are (a mixed pair runs the batch-statistics
    launches and the engine zeroes the statistics terms of the held half)."""
    assert bn_held("p.0.conv_3_1.1|conv_5_1.1", {"p.0.conv_3_1.1", "p.0.conv_5_1.1"})
    assert not bn_held("p.0.conv_3_1.1|conv_5_1.1", {"p.0.conv_3_1.1"})
    assert bn_held("conv_3_1.1|conv_5_1.1", {"conv_3_1.1", "conv_5_1.1"}) and not bn_held("conv_3_1.1|conv_5_1.1", {"conv_5_1.1"})
    full = block_backward_plan("msrb", frozenset(FZ.msrb_names()), True)
    assert block_backward_plan("msrb", frozenset(FZ.msrb_names()), True, bn_eval={"conv_3_1.1", "conv_5_2.1"}) != full
    mixed = block_backward_plan("msrb", frozenset(FZ.msrb_names()), True, bn_eval={"conv_3_1.1"})
    assert mixed == full
    both = block_backward_plan("msrb", frozenset(), True, bn_eval={"conv_3_1.1", "conv_5_1.1", "conv_3_2.1", "conv_5_2.1"})
    assert Counter(r.kind for r in both) == Counter(dgrad=6, bn_bwd_apply=3)


# ----------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_bound_and_exported_at_abi_24():
    from tactilesr_amd import _lib
    assert _lib.ABI_VERSION == 24
    lib = _lib.load()
    assert lib.tsr_abi_version() == 24
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert "nn.BatchNorm2d in EVAL mode inside a training module" in header
    # the library exports exactly what the header declares
    declared = set(re.findall(r"^\s*(?:int|long long|const int\*)\s+(tsr_\w+|tpsf_\w+)\s*\(", header, re.M))
    assert set(ENTRY_POINTS) <= declared <= set(_lib.SIGNATURES)
    # the prefix families of tests/_frozen.py keep counting the new names
    assert FZ.family("tsr_bn_bwd_apply_eval") == FZ.family("tsr_bn_bwd_apply_eval_b16") == "bn_bwd_apply"
    assert FZ.family("tsr_bn_bwd_finalize_eval") == "bn_bwd_finalize"


def test_entry_points_refuse_every_bad_argument_before_any_launch():
    """Status 1 from the host-side checks: the fake pointers are never dereferenced and no device is needed."""
    from ctypes import c_int as I, c_float as Fl
    from tactilesr_amd import _lib
    lib = _lib.load()
    fake, null = ctypes.c_void_p(256), ctypes.c_void_p(0)

    def vectors(**o):
        a = dict(dict(bias=fake, gamma=fake, beta=fake, rm=fake, rv=fake, C=64, scale=fake, shift=fake, xa=fake, xb=fake), **o)
        return lib.tsr_bn_eval_vectors(a["bias"], a["gamma"], a["beta"], a["rm"], a["rv"], Fl(1e-5), I(a["C"]), a["scale"],
                                       a["shift"], a["xa"], a["xb"], null)

    for k in ("gamma", "beta", "rm", "rv", "scale", "shift", "xa", "xb"):          # (a NULL bias is a conv without bias)
        assert vectors(**{k: null}) == 1, k
    for C in (0, -16, 8, 24, 65, 100):
        assert vectors(C=C) == 1, C

    def finalize(**o):
        a = dict(dict(slab=fake, entries=18, C=128, dg=fake, db=fake, work=fake), **o)
        return lib.tsr_bn_bwd_finalize_eval(a["slab"], I(a["entries"]), I(a["C"]), a["dg"], a["db"], a["work"], null)

    for over in (dict(slab=null), dict(dg=null), dict(db=null), dict(work=null), dict(entries=0), dict(entries=-4), dict(C=0),
                 dict(C=24), dict(C=72), dict(C=96), dict(C=256)):
        assert finalize(**over) == 1, over

    def apply(b16, **o):
        a = dict(dict(g=fake, ctot=256, coff=64, scale=fake, C=128, B=3, HW=144), **o)
        args = [a["g"], I(a["ctot"]), I(a["coff"]), a["scale"], I(a["C"]), I(a["B"]), I(a["HW"])]
        return lib.tsr_bn_bwd_apply_eval_b16(*args, null) if b16 else lib.tsr_bn_bwd_apply_eval(*args, null, null)

    bad = [dict(g=null), dict(scale=null), dict(C=0), dict(C=-16), dict(C=24), dict(C=72), dict(ctot=250), dict(ctot=0),
           dict(coff=8), dict(coff=72), dict(coff=144), dict(coff=256), dict(C=256, coff=16), dict(coff=-16), dict(coff=-64),
           dict(coff=-128, C=64), dict(B=0), dict(B=-1), dict(HW=0), dict(HW=-5), dict(HW=1 << 30)]
    for b16 in (False, True):
        for over in bad:
            assert apply(b16, **over) == 1, (b16, over)


# ----------------------------------------------------------------------------------------------------------------- glue
def test_hold_bn_statistics_survives_train_and_clears():
    import tactilesr_amd
    from tactilesr_amd.model.tactileSR_model import MSRB, ResBlock, hold_bn_statistics
    m = tactilesr_amd.TactileSR(**CFG)
    keys = list(m.state_dict())
    mods = dict(m.named_modules())
    trunk, every = set(BM.trunk_bn_paths(m)), set(BM.bn_paths(m))
    m.train()
    assert hold_bn_statistics(m.patternFeatureExtra_layer) is m.patternFeatureExtra_layer
    flags = lambda: {n for n in every if not mods[n].training}
    assert flags() == trunk
    m.train()
    assert flags() == trunk and m.training and m.patternFeatureExtra_layer[0].training
    m.eval()
    assert flags() == every
    m.train()
    assert flags() == trunk
    m.patternFeatureExtra_layer.train()               # the containers' own train() (nn.Sequential) reaches MSRB.train()
    assert flags() == trunk
    hold_bn_statistics(m.patternFeatureExtra_layer)   # marking twice keeps the first remembered mode
    hold_bn_statistics(m.patternFeatureExtra_layer, hold=False)
    assert flags() == set()
    m.train()
    assert flags() == set()
    assert list(m.state_dict()) == keys
    blk = MSRB().train()
    hold_bn_statistics(blk)
    blk.train()
    assert not any(mod.training for mod in blk.modules() if isinstance(mod, torch.nn.BatchNorm2d)) and blk.training
    assert list(blk.state_dict()) == list(MSRB().state_dict())
    hold_bn_statistics(blk, hold=False)
    assert all(mod.training for mod in blk.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    assert ResBlock().train().training                # (no BatchNorm inside: nothing to mark)


def test_model_param_init_hold_bn_marks_the_transplanted_containers():
    import tactilesr_amd
    from tactilesr_amd.train.checkpoint import model_param_init
    torch.manual_seed(0)
    cfg = dict(scale_factor=3, patternFeatureExtraLayerCnt=2, forceFeatureExtraLayerCnt=1)
    single_sd = tactilesr_amd.TactileSR(seqsCnt=1, **cfg).state_dict()
    make = lambda: tactilesr_amd.TactileSR(seqsCnt=1, **cfg)
    assert inspect.signature(model_param_init).parameters["hold_bn"].default is False
    for hold in (False, True):
        seqs = tactilesr_amd.TactileSR(seqsCnt=2, **cfg).train()
        model_param_init(seqs, single_sd, make, freeze=True, hold_bn=hold)
        seqs.train()                                  # the reference trainer's per-epoch model.train()
        held = {n for n, mod in seqs.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and not mod.training}
        assert held == (set(BM.trunk_bn_paths(seqs)) if hold else set()), hold
        assert all(p.requires_grad != FZ.is_trunk(n) for n, p in seqs.named_parameters())


def test_graphed_step_key_follows_the_batchnorm_modes():
    from tactilesr_amd.train.graph import GraphedTrainStep
    src = inspect.getsource(GraphedTrainStep._key)
    assert "BatchNorm2d" in src and ".training" in src


# ------------------------------------------------------------------------------ the engines' control flow, without a device
class _DryRun:
    """Replaces the launch functions of model/_train.py (and the layout converters' in model/tactileSR_model.py) by counters,
    so that the engines run their host code on CPU tensors: what they WOULD launch is counted by entry-point name."""

    def __enter__(self):
        from tactilesr_amd.model import _train, tactileSR_model
        self.mods = (_train, tactileSR_model)
        self.saved = [(m, k, getattr(m, k)) for m in self.mods for k in ("call", "ptr", "stream", "conv_ex") if hasattr(m, k)]
        self.names, self.conv, self.trace = Counter(), [], []          # trace: every launch in order, with its arguments

        def call(name, *args):
            self.names[name] += 1
            self.trace.append((name, args))

        def conv_ex(**kw):
            self.conv.append(kw)
            self.trace.append(("conv_ex", kw))

        for m in self.mods:
            m.call, m.ptr, m.stream = call, (lambda t: ctypes.c_void_p(0)), (lambda: ctypes.c_void_p(0))
        _train.conv_ex = conv_ex
        return self

    def __exit__(self, *exc):
        for m, k, v in self.saved:
            setattr(m, k, v)
        return False


def _dry_step(m, B=3):
    eng = m.train_engine()
    with _DryRun() as dry, torch.no_grad():
        out, c = eng.forward(torch.rand(B, 3 * m.seqsCnt, 4, 4))
        fwd, fconv = Counter(dry.names), list(dry.conv)
        dry.names.clear()
        dry.conv.clear()
        grads = eng.backward(c, torch.ones_like(out))
    return fwd, fconv, Counter(dry.names), list(dry.conv), grads, c


@pytest.mark.parametrize("impl", ["fp16x3", "bf16", "f32"])
def test_engine_host_code_all_training_issues_todays_launches(impl):
    """Every BatchNorm in training mode: no new entry point is called, every BN conv launches with its statistics epilogue."""
    m, *_ = _cpu_model()
    m.train_impl = impl
    BM.set_modes(m, [])
    fwd, fconv, bwd, bconv, grads, c = _dry_step(m)
    assert not any(n in ENTRY_POINTS for n in list(fwd) + list(bwd))
    n_bn = len(BM.bn_paths(m))
    pair = 2 if impl == "bf16" else 0                 # bf16: the stage-1 pair of each MSRB is one launch and one finalize
    assert fwd["tsr_bn_stats_finalize"] == n_bn - pair
    assert sum(1 for kw in fconv if kw.get("epi_mode") == 1) == n_bn - 2 - pair          # (the two stems' first convs are VALU)
    assert sum(bwd[k] for k in bwd if k.startswith("tsr_bn_bwd_finalize")) == 2 * 3 + 1 + 2 * 2
    assert sum(1 for kw in bconv if kw.get("bn")) == 2 * 3 + 1 + 2 * 2
    assert c.bn_eval == frozenset()


@pytest.mark.parametrize("impl", ["fp16x3", "bf16", "f32"])
@pytest.mark.parametrize("pattern", ["all", "seqs", "mixed", "stem"])
def test_engine_host_code_follows_the_held_layers(pattern, impl):
    m, *_ = _cpu_model()
    m.train_impl = impl
    held = set(BM.pattern_paths(m, pattern))
    BM.set_modes(m, held)
    if pattern == "seqs":
        for n, p in m.named_parameters():
            p.requires_grad_(not FZ.is_trunk(n))
    want = frozenset(n for n, p in m.named_parameters() if p.requires_grad)
    fwd, fconv, bwd, bconv, grads, c = _dry_step(m)
    assert c.bn_eval == frozenset(held) and set(grads) == set(want)
    n_bn, io16 = len(BM.bn_paths(m)), impl == "bf16"
    # forward: one tsr_bn_eval_vectors per held layer (one per pair launch when bf16 runs the pair and a half of it is held)
    pairs = [("patternFeatureExtra_layer.%d.conv_3_1.1" % i, "patternFeatureExtra_layer.%d.conv_5_1.1" % i) for i in range(2)]
    exp_vec, exp_fin = len(held), n_bn - len(held)
    if io16:
        for a, b in pairs:
            k = (a in held) + (b in held)
            exp_vec -= 1 if k == 2 else 0
            exp_fin -= 1 if k == 0 else 0
            # (a mixed pair still runs the one 128-channel finalize: counted once, with its training half)
    assert fwd["tsr_bn_eval_vectors"] == exp_vec and fwd.get("tsr_bn_stats_finalize", 0) == exp_fin
    stems_held = sum(1 for t in range(2) if f"inputLayer_pattern_list.{t}.2" in held)
    assert fwd.get("tsr_cb16_stats_b16" if io16 else "tsr_cb16_stats", 0) == 2 - stems_held
    plan = backward_plan(2, 2, 1, want, False, bn_eval=held)
    kinds = Counter(r.kind for r in plan)
    held_rec = [r for r in plan if r.kind == "bn_bwd_apply" and bn_held(r.layer, held)]
    ap_eval = "tsr_bn_bwd_apply_eval_b16" if io16 else "tsr_bn_bwd_apply_eval"
    ap = "tsr_bn_bwd_apply_b16" if io16 else "tsr_bn_bwd_apply"
    assert bwd.get(ap_eval, 0) == len(held_rec) and bwd.get(ap, 0) == kinds["bn_bwd_apply"] - len(held_rec)
    fin_eval = sum(1 for r in plan if r.kind == "bn_bwd_finalize" and bn_held(r.layer, held))
    assert bwd.get("tsr_bn_bwd_finalize_eval", 0) == fin_eval
    assert bwd.get("tsr_bn_bwd_finalize", 0) == kinds["bn_bwd_finalize"] - fin_eval
    # a dgrad leaves BatchNorm sums exactly when the plan says so
    assert sum(1 for kw in bconv if kw.get("bn")) == sum(1 for r in plan if r.kind == "dgrad" and any(t.endswith(".sums") for t in r.produces))
    assert len(bconv) == kinds["dgrad"]
    if pattern == "seqs":
        assert fin_eval == 0 and len(held_rec) == 2 * 3
        assert sum(1 for kw in bconv if kw.get("bn")) == 1 + 2 * 2          # inputContact_layer.1 and the stems only
    # forward convs of held layers ask for no statistics epilogue (the bf16 pair form only knows epi_mode 1)
    epi1 = sum(1 for kw in fconv if kw.get("epi_mode") == 1)
    exp_epi1 = (n_bn - 2) - len([h for h in held if not h.endswith("pattern_list.0.2") and not h.endswith("pattern_list.1.2")])
    if io16:
        for a, b in pairs:
            k = (a in held) + (b in held)
            exp_epi1 += {0: -1, 1: 0, 2: 1}[k]        # one launch for the two layers; kept in epi_mode 1 even when both are held
    assert epi1 == exp_epi1, (epi1, exp_epi1)


@pytest.mark.parametrize("impl", ["fp16x3", "bf16", "f32"])
def test_statistics_are_reduced_over_the_entries_of_the_launch_that_wrote_them(impl):
    """Every launch that leaves per-workgroup sums in the statistics slab is followed by a finalize over exactly the entries
    the library reports for the form (`nsplit`) that was launched.  B = 5: a form with 2 images per workgroup and one with 4
    differ there (6 and 8 entries per tile), at B = 3 they would not.  One layer is held so that both backward finalizes run."""
    import tactilesr_amd
    from tactilesr_amd import _lib
    torch.manual_seed(5)
    m = tactilesr_amd.TactileSR(3, 2, 3, 2, 1).train()
    m.train_impl = impl
    m.patternFeatureExtra_layer[0].conv_3_2[1].eval()
    B, H, W = 5, 12, 12
    eng = m.train_engine()
    with _DryRun() as dry, torch.no_grad():
        out, c = eng.forward(torch.rand(B, 6, 4, 4))
        eng.backward(c, torch.ones_like(out))
    assert out.shape == (B, 1, H, W)
    want = lambda kw: _lib.load().tsr_conv2d_slab_entries_ex(B, H, W, kw["cout"], kw["ks"], kw["nsplit"])

    def following(i, names):
        for name, args in dry.trace[i + 1:]:
            assert name != "conv_ex", "no finalize between two conv launches"
            if name in names:
                return name, args

    seen = Counter()
    for i, (name, kw) in enumerate(dry.trace):
        if name != "conv_ex":
            continue
        if kw.get("epi_mode") == 1:
            fin, args = following(i, ("tsr_bn_stats_finalize",))
            assert args[2].value == want(kw), (kw["cout"], kw["ks"], kw["nsplit"])
            seen[fin] += 1
        if kw.get("bn"):
            fin, args = following(i, ("tsr_bn_bwd_finalize", "tsr_bn_bwd_finalize_eval"))
            assert args[1].value == want(kw), (kw["cout"], kw["ks"], kw["nsplit"])
            seen[fin] += 1
    pair = 2 if impl == "bf16" else 0
    assert seen == Counter(tsr_bn_stats_finalize=2 + 1 + 4 * 2 - 1 - pair, tsr_bn_bwd_finalize=2 * 3 + 1 + 2 * 2 - 1,
                           tsr_bn_bwd_finalize_eval=1)


@pytest.mark.parametrize("held", [("conv_3_1.1", "conv_5_1.1", "conv_3_2.1", "conv_5_2.1"), ("conv_5_1.1", "conv_3_2.1")])
def test_block_engine_inherits_the_behaviour(held):
    from tactilesr_amd.model.tactileSR_model import MSRB
    torch.manual_seed(3)
    blk = MSRB().train()
    mods = dict(blk.named_modules())
    for n in held:
        mods[n].eval()
    eng = blk.block_engine()
    with _DryRun() as dry, torch.no_grad():
        out, c = eng.forward(torch.rand(2, 64, 6, 6))
        fwd = Counter(dry.names)
        dry.names.clear()
        grads = eng.backward(c, torch.ones_like(out))
        dx = c.dx
    assert c.bn_eval == frozenset(held)
    assert fwd["tsr_bn_eval_vectors"] == len(held) and fwd.get("tsr_bn_stats_finalize", 0) == 4 - len(held)
    plan = block_backward_plan("msrb", c.want, True, bn_eval=held)
    n_held = sum(1 for r in plan if r.kind == "bn_bwd_apply" and bn_held(r.layer, held))
    assert dry.names.get("tsr_bn_bwd_apply_eval", 0) == n_held == (3 if len(held) == 4 else 1)
    assert dry.names.get("tsr_bn_bwd_apply", 0) == 3 - n_held
    assert set(grads) == set(c.want) and dx is not None
