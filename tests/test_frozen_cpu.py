"""Host-side tests of frozen parameters in the train step: the backward plan (which launches a want-set keeps), the
gradient arena / sink / sync with a reduced want-set (on a toy engine, like tests/test_ddp_cpu.py), the two head data-gradient
entry points' declaration and refusals, and ``model_param_init(freeze=True)``."""
import os
import random
import re
import socket
from collections import Counter

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tactilesr_amd.model._train import backward_plan, block_backward_plan

import _frozen as FZ

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the plan
def test_helper_names_are_the_models():
    """tests/_frozen.py derives parameter names from the architecture: they are the module's own."""
    import tactilesr_amd
    from tactilesr_amd.model.tactileSR_model import MSRB, ResBlock
    for T, M, R in ((1, 2, 1), (2, 3, 2)):
        m = tactilesr_amd.TactileSR(3, T, 3, M, R)
        assert sorted(FZ.param_names(T, M, R)) == sorted(n for n, _ in m.named_parameters())
        bn = {n + "." + k for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) for k in ("weight", "bias")}
        assert {n for n in FZ.param_names(T, M, R) if FZ.is_bn(n)} == bn
    assert sorted(FZ.msrb_names()) == sorted(n for n, _ in MSRB().named_parameters())
    assert sorted(FZ.res_names()) == sorted(n for n, _ in ResBlock().named_parameters())


def test_full_plan_is_todays_launch_list():
    """want = every parameter: the unfiltered list.  Counted from TrainEngine.backward for M = 2, R = 1, T = 1:
      wgrad           output_layer.0 (1) + ResBlock conv2, conv1 (2) + per MSRB confusion, conv_3_2, conv_5_2, conv_3_1, conv_5_1
                      (5 x 2) + inputContact_layer.0 (1) + the stem's second conv seq[4] (1)                          = 15
      dgrad           output_layer.0 (1) + ResBlock (2) + per MSRB two confusion halves, two stage-2, two stage-1 (6 x 2) +
                      one inputContact_layer.0 slice per frame (1) + seq[4] (1)                                        = 17
      bn_bwd_finalize per MSRB conv_3_2.1, conv_5_2.1, the stage-1 pair (3 x 2) + inputContact_layer.1 + seq[5], seq[2]  = 9
                      (each with its bn_bwd_apply)
      stem_wgrad      input_layer_force.1 + the frame's seq[1]                                                         = 2
      head_bwd        1, and no head_dgrad
      tsr_reduce_splits: head (1) + output_layer.0 weight (1) + ResBlock weight, bias x 2 (4) + MSRB weight, bias x 5 x 2
                      (20) + inputContact_layer.0 (1) + seq[4] (1) + two stems (2)                                     = 30"""
    names = FZ.param_names(1, 2, 1)
    plan = backward_plan(1, 2, 1, frozenset(names), False)
    k = Counter(r.kind for r in plan)
    assert k == Counter(wgrad=15, dgrad=17, bn_bwd_finalize=9, bn_bwd_apply=9, stem_wgrad=2, head_bwd=1)
    assert FZ.expected_calls(plan, frozenset(names))["reduce_splits"] == 30
    assert sorted(n for r in plan for n in r.params) == sorted(names)          # every parameter exactly once
    assert len({r.key for r in plan}) == len(plan)
    # with the taxel gradient: the same list plus one stem_dgrad behind each stem_wgrad
    pdx = backward_plan(1, 2, 1, frozenset(names), True)
    assert [r for r in pdx if r.kind != "stem_dgrad"] == plan
    assert [pdx[i - 1].key for i, r in enumerate(pdx) if r.kind == "stem_dgrad"] == \
        [("stem_wgrad", "input_layer_force.1"), ("stem_wgrad", "inputLayer_pattern_list.0.1")]
    # the head of the list, in the engine's order
    assert [r.key for r in plan[:5]] == [("head_bwd", "output_layer.2"), ("wgrad", "output_layer.0"),
                                         ("dgrad", "output_layer.0"), ("wgrad", "forceFeatureExtra_layer.0.conv2"),
                                         ("dgrad", "forceFeatureExtra_layer.0.conv2")]


def test_empty_want_is_an_empty_plan():
    assert backward_plan(2, 3, 2, frozenset(), False) == []
    assert block_backward_plan("msrb", frozenset(), False) == []
    assert block_backward_plan("res", frozenset(), False) == []


def _slot(r):
    """A launch's identity across plans: head_bwd and head_dgrad are the two forms of the one head launch."""
    return ("head" if r.kind in ("head_bwd", "head_dgrad") else r.kind), r.layer


def _is_subsequence(a, b):
    it = iter(b)
    return all(x in it for x in a)


def test_random_subsets_are_closed_minimal_and_monotone():
    T, M, R = 2, 3, 2
    names = FZ.param_names(T, M, R)
    rng = random.Random(20240)
    for trial in range(200):
        k = rng.choice((1, 2, 3, 5, 10, 40, len(names)))
        A = frozenset(rng.sample(names, min(k, len(names))))
        want_dx = rng.random() < 0.3
        plan = backward_plan(T, M, R, A, want_dx)
        produced, params = set(), Counter()
        for r in plan:
            for lab in r.consumes:          # produced by an earlier record, or a tensor the forward saved
                assert lab in produced or lab.startswith("saved:"), (trial, r, lab)
            produced.update(r.produces)
            params.update(n for n in r.params if n in A)
        assert params == Counter(A), trial                                   # every wanted name exactly once
        consumed = {lab for r in plan for lab in r.consumes}
        for r in plan:                                                       # nobody is present without a taker
            used = (any(n in A for n in r.params) or any(lab in consumed for lab in r.produces)
                    or (r.kind == "stem_dgrad" and want_dx))
            assert used, (trial, r)
            assert r.kind != "head_dgrad" or "output_layer.2.weight" not in A
            assert r.kind != "head_bwd" or "output_layer.2.weight" in A
        Bset = frozenset(rng.sample(names, rng.choice((1, 4, 30))))
        bigger = backward_plan(T, M, R, A | Bset, want_dx or rng.random() < 0.5)
        assert _is_subsequence([_slot(r) for r in plan], [_slot(r) for r in bigger]), trial


def _kinds(plan):
    return Counter(r.kind for r in plan)


def test_pattern_head_only():
    names = FZ.param_names(2, 3, 1)
    want, dx = FZ.PATTERNS["head"](names)
    assert [r.key for r in backward_plan(2, 3, 1, want, dx)] == [("head_bwd", "output_layer.2"), ("wgrad", "output_layer.0")]


def test_pattern_trunk_frozen():
    T = 2
    names = FZ.param_names(T, 3, 1)
    want, dx = FZ.PATTERNS["trunk"](names)
    plan, full = backward_plan(T, 3, 1, want, dx), backward_plan(T, 3, 1, frozenset(names), False)
    assert [r.layer for r in plan if r.kind == "wgrad"] == ["output_layer.0", "inputContact_layer.0",
                                                            "inputLayer_pattern_list.0.4", "inputLayer_pattern_list.1.4"]
    assert [r for r in plan if r.kind == "dgrad"] == [r for r in full if r.kind == "dgrad"]
    assert _kinds(plan)["head_bwd"] == 1 and _kinds(plan)["stem_wgrad"] == T + 1
    # BatchNorm layers of the frozen MSRBs: every apply pass stays (dz is consumed), and so does its finalize
    assert _kinds(plan)["bn_bwd_apply"] == _kinds(full)["bn_bwd_apply"]


def test_pattern_all_frozen_with_input_grad():
    T = 2
    plan = backward_plan(T, 3, 1, frozenset(), True)
    k = _kinds(plan)
    assert k["wgrad"] == 0 and k["stem_wgrad"] == 0 and k["head_bwd"] == 0
    assert k["head_dgrad"] == 1 and k["stem_dgrad"] == T + 1
    assert FZ.expected_calls(plan, frozenset())["reduce_splits"] == 0


def test_pattern_middle_msrb_only():
    names = FZ.param_names(1, 3, 1)
    want, dx = FZ.PATTERNS["middle_msrb"](names)
    plan = backward_plan(1, 3, 1, want, dx)
    layers = [r.layer for r in plan]
    assert not any(l.startswith(("forceFeatureExtra_layer", "input_layer_force", "patternFeatureExtra_layer.0",
                                 "inputContact_layer", "inputLayer_pattern_list")) for l in layers)
    assert not any(r.kind == "wgrad" and r.layer.startswith("patternFeatureExtra_layer.2") for r in plan)
    assert sum(r.kind == "wgrad" for r in plan) == 5                       # block 1's own
    assert ("dgrad", "patternFeatureExtra_layer.1.conv_5_1.0") not in {r.key for r in plan}      # nobody takes its dx
    assert plan[0].key == ("head_dgrad", "output_layer.2")


def test_pattern_batchnorm_only():
    names = FZ.param_names(2, 3, 1)
    want, dx = FZ.PATTERNS["bn_only"](names)
    plan = backward_plan(2, 3, 1, want, dx)
    k = _kinds(plan)
    assert k["wgrad"] == 0 and k["stem_wgrad"] == 0 and k["head_bwd"] == 0 and k["head_dgrad"] == 1
    assert k["bn_bwd_finalize"] == 3 * 3 + 1 + 2 * 2
    # the stems' first BatchNorm ends the chain: its dgamma / dbeta need the finalize, nobody needs its dz
    assert k["bn_bwd_apply"] == k["bn_bwd_finalize"] - 2
    assert not any(r.layer.startswith("forceFeatureExtra_layer") for r in plan)


def test_frozen_weight_with_trainable_bias_keeps_the_wgrad_launch():
    names = FZ.param_names(1, 2, 1)
    want = frozenset({"forceFeatureExtra_layer.0.conv1.bias"})
    plan = backward_plan(1, 2, 1, want, False)
    assert [r.key for r in plan] == [("head_dgrad", "output_layer.2"), ("dgrad", "output_layer.0"),
                                     ("dgrad", "forceFeatureExtra_layer.0.conv2"),
                                     ("wgrad", "forceFeatureExtra_layer.0.conv1")]
    assert FZ.expected_calls(plan, want)["reduce_splits"] == 1
    want, dx = FZ.PATTERNS["res_bias"](names)
    plan = backward_plan(1, 2, 1, want, dx)
    assert {("wgrad", "forceFeatureExtra_layer.0.conv1"), ("wgrad", "forceFeatureExtra_layer.0.conv2")} <= {r.key for r in plan}
    assert FZ.expected_calls(plan, want)["reduce_splits"] == 30 - 2


def test_standalone_block_plans():
    full = block_backward_plan("msrb", frozenset(FZ.msrb_names()), True)
    assert _kinds(full) == Counter(wgrad=5, dgrad=6, bn_bwd_finalize=3, bn_bwd_apply=3)
    assert not any(lab.endswith("dx.sums") for r in full for lab in r.produces)       # a plain input: no BatchNorm below
    # a frozen conv_3_2 and an input without grad: its wgrad goes, the stage-1 dgrads (dx) go
    want = frozenset(n for n in FZ.msrb_names() if not n.startswith("conv_3_2.0."))
    plan = block_backward_plan("msrb", want, False)
    assert [r.layer for r in plan if r.kind == "wgrad"] == ["confusion", "conv_5_2.0", "conv_3_1.0", "conv_5_1.0"]
    assert [r.layer for r in plan if r.kind == "dgrad"] == ["confusion[0:128]", "confusion[128:256]", "conv_3_2.0", "conv_5_2.0"]
    full = block_backward_plan("res", frozenset(FZ.res_names()), True)
    assert [r.key for r in full] == [("wgrad", "conv2"), ("dgrad", "conv2"), ("wgrad", "conv1"), ("dgrad", "conv1")]
    assert [r.key for r in block_backward_plan("res", frozenset({"conv2.weight", "conv2.bias"}), False)] == [("wgrad", "conv2")]
    assert [r.key for r in block_backward_plan("res", frozenset(), True)] == [("dgrad", "conv2"), ("dgrad", "conv1")]


# ------------------------------------------------------------------------------------------- arena, sink, sync on a toy
class _ToyEngine:
    """Stands in for TrainEngine: three linear pieces whose gradients appear in reverse layer order through a GradSink
    that is told the want-set; a gradient nobody wants is not produced."""

    def __init__(self, module):
        self.m = module
        self.arena = None
        self.grad_sync = None
        self.n_buckets = 3
        self.modes = []

    def backward(self, x, dy, want, token):
        from tactilesr_amd.ddp import GradSink
        sink = GradSink(self, dict(self.m.named_parameters()), x.device, token=token, want=want)
        self.modes.append("first" if sink.first else "direct" if sink.direct else "shared" if sink.shared else "accum")
        for name in ("l3", "l2", "l1"):
            lin = getattr(self.m, name)
            if f"{name}.weight" in want:
                gw = sink.dest(f"{name}.weight", lin.weight.shape)
                torch.matmul(dy.t(), x, out=gw)
                sink.put(f"{name}.weight", gw)
            if f"{name}.bias" in want:
                sink.put_copy(f"{name}.bias", dy.sum(0))
        return sink.finalize()


class _Token:
    pass


class _ToyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, names, x, *params):
        m = engine.m
        ctx.engine, ctx.names, ctx.x = engine, names, x
        ctx.want = frozenset(n for n, need in zip(names, ctx.needs_input_grad[3:]) if need)
        ctx.token = _Token()
        if any(ctx.needs_input_grad):
            from tactilesr_amd.ddp import note_forward
            note_forward(engine, ctx.token)
        return sum(x @ l.weight.t() + l.bias for l in (m.l1, m.l2, m.l3))

    @staticmethod
    def backward(ctx, dy):
        g = ctx.engine.backward(ctx.x, dy.contiguous(), ctx.want, ctx.token)
        return (None, None, None) + tuple(g.get(n) if n in ctx.want else None for n in ctx.names)


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.l1, self.l2, self.l3 = (torch.nn.Linear(40, 24) for _ in range(3))
        self._engine = _ToyEngine(self)

    def train_engine(self):
        return self._engine

    def forward(self, x):
        named = list(self.named_parameters())
        return _ToyFn.apply(self._engine, [n for n, _ in named], x, *[p for _, p in named])


def _toy_step(m, x, fired=None):
    for p in m.parameters():
        if p.requires_grad:
            p.grad = None
    m(x).pow(2).mean().backward()


def test_changed_want_set_relays_the_arena_and_stale_frozen_grad_keeps_direct():
    torch.manual_seed(3)
    m = _Toy()
    eng = m.train_engine()
    x = torch.randn(6, 40)
    named = dict(m.named_parameters())
    _toy_step(m, x)
    _toy_step(m, x)
    a0 = eng.arena
    assert eng.modes == ["first", "direct"]
    assert a0.names == ["l3.weight", "l3.bias", "l2.weight", "l2.bias", "l1.weight", "l1.bias"]
    ref = {n: p.grad.clone() for n, p in named.items()}
    # freeze l2: its stale .grad stays where it is (no optimizer clears it), the arena is laid out again without it
    for n in ("l2.weight", "l2.bias"):
        named[n].requires_grad_(False)
    stale = named["l2.weight"].grad
    assert stale is not None
    _toy_step(m, x)
    a1 = eng.arena
    assert eng.modes[-1] == "first" and a1 is not a0
    assert a1.names == ["l3.weight", "l3.bias", "l1.weight", "l1.bias"] and a1.total < a0.total
    fired = []
    a1.on_bucket_ready = lambda k, flat: fired.append((k, a1._members[k]))
    _toy_step(m, x)
    # direct although a frozen parameter still carries a .grad; buckets fire with the reduced member count
    assert eng.modes[-1] == "direct" and named["l2.weight"].grad is stale
    assert [k for k, _ in fired] == list(range(len(a1.buckets))) and sum(n for _, n in fired) == 4
    for n in a1.names:
        assert named[n].grad.data_ptr() == a1.flat.data_ptr() + 4 * a1.offsets[n], n
        assert torch.equal(named[n].grad, ref[n]), n
    # a stale .grad on a WANTED parameter is gradient accumulation, as before
    m(x).pow(2).mean().backward()
    assert eng.modes[-1] == "accum"
    # unfreezing lays the arena out once more
    for n in ("l2.weight", "l2.bias"):
        named[n].requires_grad_(True)
        named[n].grad = None
    _toy_step(m, x)
    assert eng.modes[-1] == "first" and eng.arena.names == a0.names


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _hash_worker(rank, world, port, q, differ):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from tactilesr_amd import ddp
    ddp.init_distributed("gloo")
    torch.manual_seed(5)
    m = _Toy()
    sync = ddp.GradSync(m)
    named = dict(m.named_parameters())
    if differ and rank == 1:
        named["l2.bias"].requires_grad_(False)
    x = torch.randn(4, 40)
    res = {"rank": rank, "error": None}
    try:
        m(x).pow(2).mean().backward()          # the first backward lays the arena out and binds it: the layouts are compared
        sync.finish()
        res["names"] = list(m.train_engine().arena.names)
    except RuntimeError as e:
        res["error"] = str(e)
    q.put(res)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("differ", [False, True])
def test_gradsync_world2_refuses_ranks_that_froze_different_sets(differ):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_hash_worker, args=(r, 2, port, q, differ)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(2)), key=lambda r: r["rank"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    if not differ:
        assert all(r["error"] is None and len(r["names"]) == 6 for r in res), res
        return
    # rank 0 holds l2.bias where rank 1 already holds l1.weight: both ranks refuse, each naming its own entry there
    assert all(r["error"] is not None and "GradSync" in r["error"] for r in res), res
    assert "'l2.bias'" in res[0]["error"] and "rank 1" in res[0]["error"]
    assert "'l1.weight'" in res[1]["error"] and "rank 0" in res[1]["error"]


# --------------------------------------------------------------------------------------------------------------- C ABI
def test_head_dgrad_entry_points_are_declared_bound_and_exported_at_abi_24():
    from tactilesr_amd import _lib
    P, I = _lib._P, _lib._I
    assert _lib.ABI_VERSION == 24
    lib = _lib.load()
    assert lib.tsr_abi_version() == 24
    bwd = _lib.SIGNATURES["tsr_head_bwd"]
    # tsr_head_bwd's arguments minus wslab / nsplit (positions 8, 9)
    assert _lib.SIGNATURES["tsr_head_dgrad"] == bwd[:8] + bwd[10:] == [P, P, P, I, I, P, P, I, I, I, I, P, P]
    b16 = _lib.SIGNATURES["tsr_head_bwd_b16"]
    assert _lib.SIGNATURES["tsr_head_dgrad_b16"] == b16[:8] + b16[10:]
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    for name in ("tsr_head_dgrad", "tsr_head_dgrad_b16"):
        assert hasattr(lib, name)
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert "model/tactileSR_model.py:55-56" in header[header.index("tsr_head_bwd("):header.index("tsr_head_dgrad_b16(")]


def test_head_dgrad_refuses_every_bad_argument_before_any_launch():
    """Status 1 from the host-side checks: the fake pointers are never dereferenced and no device is needed.  The refusals
    are tsr_head_bwd's without the wslab / nsplit ones and without the (H + 2)(W + 2) LDS bound (the weight gradient's)."""
    import ctypes
    from ctypes import c_int as I
    from tactilesr_amd import _lib
    lib = _lib.load()
    fake, null = ctypes.c_void_p(256), ctypes.c_void_p(0)
    good = dict(dout=fake, out=fake, h0=fake, h_ctot=128, cin=128, w=fake, dz=fake, dz_ctot=128, B=2, H=12, W=12)

    def status(b16, **over):
        a = dict(good, **over)
        args = [a["dout"], a["out"], a["h0"], I(a["h_ctot"]), I(a["cin"]), a["w"], a["dz"], I(a["dz_ctot"]), I(a["B"]),
                I(a["H"]), I(a["W"])]
        if b16:
            return lib.tsr_head_dgrad_b16(*args, null)
        return lib.tsr_head_dgrad(*args, null, null)

    bad = [dict(dout=null), dict(out=null), dict(h0=null), dict(w=null), dict(dz=null), dict(cin=24), dict(cin=272, h_ctot=272,
           dz_ctot=272), dict(h_ctot=112), dict(dz_ctot=112), dict(h_ctot=136), dict(dz_ctot=136), dict(B=0), dict(B=-1),
           dict(H=0), dict(W=0), dict(H=-3), dict(H=1 << 15, W=1 << 15)]
    for b16 in (False, True):
        for over in bad:
            assert status(b16, **over) == 1, (b16, over)


# ---------------------------------------------------------------------------------------------------------------- glue
def test_model_param_init_freeze_flags_exactly_the_transplanted_parameters():
    import tactilesr_amd
    from tactilesr_amd.train.checkpoint import model_param_init
    torch.manual_seed(0)
    cfg = dict(scale_factor=3, patternFeatureExtraLayerCnt=2, forceFeatureExtraLayerCnt=1)
    single_sd = tactilesr_amd.TactileSR(seqsCnt=1, **cfg).state_dict()
    make = lambda: tactilesr_amd.TactileSR(seqsCnt=1, **cfg)
    for freeze in (False, True):
        seqs = tactilesr_amd.TactileSR(seqsCnt=2, **cfg)
        before = {id(p) for p in seqs.parameters()}
        out = model_param_init(seqs, single_sd, make, freeze=freeze) if freeze else model_param_init(seqs, single_sd, make)
        assert out is seqs
        for n, p in seqs.named_parameters():
            assert p.requires_grad == (not (freeze and FZ.is_trunk(n))), (freeze, n)
            assert (id(p) not in before) == FZ.is_trunk(n), n                 # the transplanted ones are new objects
        for k, v in seqs.state_dict().items():
            if FZ.is_trunk(k):
                assert torch.equal(v, single_sd[k]), k
    assert "reference" in model_param_init.__doc__ and "clip_grad_norm_" in model_param_init.__doc__


def test_graphed_step_key_follows_requires_grad_and_refuses_nothing_to_train():
    """Host-only part of the GraphedTrainStep change: the source of `_key` carries the requires_grad tuple, and `_check`
    refuses a model without a trainable parameter before looking at anything on a device."""
    import inspect
    from tactilesr_amd._lib import TactileSRHipError
    from tactilesr_amd.train.graph import GraphedTrainStep
    assert "requires_grad" in inspect.getsource(GraphedTrainStep._key)

    class _M(torch.nn.Module):
        training = True

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(2), requires_grad=False)

    g = GraphedTrainStep.__new__(GraphedTrainStep)
    g.model = _M()
    with pytest.raises(TactileSRHipError, match="requires grad"):
        g._check(torch.zeros(1), torch.zeros(1))


# ------------------------------------------------------------------------------- the engines' control flow, without a device
class _DryRun:
    """Replaces the launch functions of model/_train.py (and the layout converters' in model/tactileSR_model.py) by counters,
    so that TrainEngine / BlockEngine run their host code on CPU tensors: what they WOULD launch is counted, nothing runs."""

    def __enter__(self):
        import ctypes
        from tactilesr_amd.model import _train, tactileSR_model
        self.mods = (_train, tactileSR_model)
        self.saved = [(m, k, getattr(m, k)) for m in self.mods for k in ("call", "ptr", "stream", "conv_ex") if hasattr(m, k)]
        self.counts = Counter()

        def call(name, *args):
            fam = FZ.family(name)
            if fam is not None:
                self.counts[fam] += 1

        def conv_ex(**kw):
            self.counts["conv_ex"] += 1

        for m in self.mods:
            m.call, m.ptr, m.stream = call, (lambda t: ctypes.c_void_p(0)), (lambda: ctypes.c_void_p(0))
        _train.conv_ex = conv_ex
        return self

    def __exit__(self, *exc):
        for m, k, v in self.saved:
            setattr(m, k, v)
        return False


@pytest.mark.parametrize("impl", ["fp16x3", "bf16", "f32"])
@pytest.mark.parametrize("pattern", list(FZ.PATTERNS))
def test_train_engine_host_code_follows_the_plan(pattern, impl):
    """No device: the engine's backward, driven directly on CPU tensors with its launch functions counted instead of run,
    asks for exactly the plan's launches, hands out exactly the wanted gradients, and lays the arena out in plan order."""
    import tactilesr_amd
    T, Mb = 2, 3
    torch.manual_seed(1)
    m = tactilesr_amd.TactileSR(3, T, 3, Mb, 1).train()
    m.train_impl = impl
    named = dict(m.named_parameters())
    want, want_dx = FZ.PATTERNS[pattern](list(named))
    for n, p in named.items():
        p.requires_grad_(n in want)
    plan = backward_plan(T, Mb, 1, want, want_dx)
    eng = m.train_engine()
    with _DryRun() as dry, torch.no_grad():
        out, c = eng.forward(torch.rand(3, 3 * T, 4, 4))
        assert c.want == want                                  # driven directly: derived from requires_grad
        c.want_dx = want_dx
        dry.counts.clear()
        grads = eng.backward(c, torch.ones_like(out))
    assert dry.counts == FZ.expected_calls(plan, want), (dry.counts, FZ.expected_calls(plan, want))
    assert set(grads) == set(want)
    assert (c.dx is not None) == want_dx
    if want:
        assert eng.arena.names == FZ.production_order(plan, want)
    else:
        assert eng.arena is None


@pytest.mark.parametrize("kind,frozen,x_grad", [("msrb", (), True), ("msrb", ("conv_3_2.0.weight", "conv_3_2.0.bias"), False),
                                                ("msrb", ("conv_5_1.0.weight",), True), ("res", (), True),
                                                ("res", ("conv1.weight", "conv1.bias"), False), ("res", ("conv2.weight",), True)])
def test_block_engine_host_code_follows_the_plan(kind, frozen, x_grad):
    from tactilesr_amd.model.tactileSR_model import MSRB, ResBlock
    torch.manual_seed(2)
    blk = (MSRB if kind == "msrb" else ResBlock)().train()
    named = dict(blk.named_parameters())
    want = frozenset(n for n in named if n not in frozen)
    for n in frozen:
        named[n].requires_grad_(False)
    plan = block_backward_plan(kind, want, x_grad)
    eng = blk.block_engine()
    with _DryRun() as dry, torch.no_grad():
        out, c = eng.forward(torch.rand(2, 64, 6, 6))
        assert c.want == want and c.want_dx is True
        c.want_dx = x_grad
        dry.counts.clear()
        grads = eng.backward(c, torch.ones_like(out))
        dx = c.dx
    assert dry.counts == FZ.expected_calls(plan, want), (dry.counts, FZ.expected_calls(plan, want))
    assert set(grads) == set(want) and (dx is not None) == x_grad
    assert eng.arena.names == FZ.production_order(plan, want)
