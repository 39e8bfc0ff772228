"""The in-backward gradient buckets on every path of the train engines, against a peer whose gradient differs.

``GradSync`` (tactilesr_amd/ddp.py) hands a bucket to the all-reduce the moment its last gradient is ``put`` -- safe only if
every backward path of model/_train.py calls ``put`` after the last launch that writes the slot has been enqueued, writes
nothing there afterwards, puts every wanted name once and no other.  On one GPU a violation changes nothing; on several it
averages a half-finished gradient.  tests/_bucket_peer.py simulates the second rank in this process (no process group, no
spawn): the all-reduce is a function that adds the PEER'S gradient -- the plain gradient of another seeded batch on a fresh
model -- to exactly the range it is handed, at call time on the current stream.  tests/test_bucket_peer_cpu.py shows on toy
engines that each kind of violation is reported.

After every backward + ``finish()``: the arena holds exactly the want-set, every wanted name was put once and no other, a
direct step shipped buckets 0 .. nb-1 in order from inside backward (every other kind nothing), every trainable ``p.grad`` is
``(local + peer) / 2`` bit for bit and aliases its slot, what a bucket held when it was shipped is the finished local gradient,
frozen parameters have no gradient, no NaN of the canary (the arena is NaN-filled before every direct backward) is left.

All cases but the arithmetic and bucket-count ones run with one bucket per tensor (``PER_TENSOR``): every ``put`` then ships
at once, so an early ``put`` cannot hide in the middle of a bucket (tests/test_bucket_peer_cpu.py shows that it can)."""
import pytest
import torch
import torch.nn.functional as F

import tactilesr_amd
from oracle import tactilesr_oracle as O
from tactilesr_amd.model import _train

import _block_cases as BC
import _bn_modes as BM
import _bucket_peer as BP
import _frozen as FZ

pytestmark = pytest.mark.gpu

_SD = {}


def _state(cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _SD:
        _SD[key] = O.random_state_dict(O.tactilesr_state_shapes(**cfg), 4100 + 7 * cfg["seqsCnt"] + cfg["scale_factor"])
    return _SD[key]


def tsr_case(T, Mb, R, impl, pattern="all", held="none", dx=None, sf=3, B=3):
    """TactileSR(seqsCnt=T, Mb MSRBs, R ResBlocks) at 4sf x 4sf with the freeze pattern `pattern` of tests/_frozen.py and the
    held-BatchNorm pattern `held` of tests/_bn_modes.py (its "seqs" freezes the two trunk containers as well)."""
    cfg = dict(scale_factor=sf, seqsCnt=T, patternFeatureExtraLayerCnt=Mb, forceFeatureExtraLayerCnt=R)
    want, want_dx = FZ.PATTERNS[pattern](FZ.param_names(T, Mb, R))
    if held == "seqs":
        want = frozenset(n for n in want if not FZ.is_trunk(n))
    dx = want_dx if dx is None else dx

    def flags(m):
        BM.set_modes(m, BM.pattern_paths(m, held))
        for n, p in m.named_parameters():
            p.requires_grad_(n in want)

    def build():
        m = tactilesr_amd.TactileSR(**cfg)
        m.train_impl = impl
        m.load_state_dict(_state(cfg), strict=True)
        m = m.cuda()
        flags(m)
        return m

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        LR = (torch.rand(B, 3 * T, 4, 4, generator=g) * 8).cuda().requires_grad_(dx)
        HR = (torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25).cuda()
        return LR, HR

    return BP.Case(("tsr", sf, T, Mb, R, B, impl, pattern, held, dx), build, lambda m: m.train_engine(), batch,
                   lambda m, b: F.mse_loss(m(b[0]), b[1]), flags=flags, dx=dx)


def block_case(kind, impl, frozen=(), x_grad=True):
    """A standalone MSRB / ResBlock through ``block_engine()`` at the (3, 8, 8) size of tests/_block_cases.py."""
    def build():
        blk, _ = BC.make_block(kind)
        blk.train_impl = impl
        blk = blk.cuda().train()
        for n, p in blk.named_parameters():
            p.requires_grad_(n not in frozen)
        return blk

    def batch(seed):
        x, dy = BC.block_data(kind, 3, 8, 8, seed=seed)
        return x.cuda().requires_grad_(x_grad), dy.cuda()

    return BP.Case(("block", kind, impl, tuple(frozen), x_grad), build, lambda b: b.block_engine(), batch,
                   lambda b, d: (b(d[0]) * d[1]).sum(), dx=x_grad)


def _run(case, monkeypatch, long=False, n_buckets=BP.PER_TENSOR):
    rig, fails = BP.run_sequence(case, monkeypatch, long=long, n_buckets=n_buckets)
    assert not fails, fails
    kinds = [k for k, _ in rig.steps]
    assert kinds == (["first", "direct", "direct"] + (["accum", "no_sync", "shared", "direct", "pending", "flat"] if long else []))
    assert not torch.distributed.is_initialized()          # no process group was opened
    return rig


def _stage1_bn(prefix=""):
    return {f"{prefix}conv_{k}_1.1.{w}" for k in (3, 5) for w in ("weight", "bias")}


# ------------------------------------------------------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("impl", list(_train.TRAIN_IMPLS))
def test_every_arithmetic(monkeypatch, impl):
    """(1, 1, 1) at the default eight buckets; fp16x3 runs the long sequence.  The sink calls of a direct step are the three
    production forms of the engine: tsr_reduce_splits into a `dest` slot, BatchNorm dgamma / dbeta written into `dest` slots by
    the finalize launch, and `put_copy` for the stage-1 pair."""
    rig = _run(tsr_case(1, 1, 1, impl), monkeypatch, long=impl == "fp16x3", n_buckets=8)
    mode, calls = rig.sink_calls[1]
    assert mode == "direct"
    names = FZ.param_names(1, 1, 1)
    assert {n for c, n in calls if c == "put_copy"} == _stage1_bn("patternFeatureExtra_layer.0.")
    via_dest = [n for c, n in calls if c == "dest"]
    assert sorted(via_dest + [n for c, n in calls if c == "put_copy"]) == sorted(names)
    assert [n for c, n in calls if c != "dest"] == rig.engine.arena.names          # put in the arena's order
    assert 2 <= len(rig.engine.arena.buckets) <= 8


class _EarlyPut:
    """A sink proxy that ticks a slot off the moment it is handed out: `put` BEFORE the launch that writes it."""

    def __init__(self, sink):
        self.sink = sink

    def dest(self, name, shape):
        t = self.sink.dest(name, shape)
        self.sink.put(name, t)
        return t

    def put(self, name, t):
        pass


def test_an_early_put_in_the_real_engine_is_reported(monkeypatch):
    """The device-side counterpart of tests/test_bucket_peer_cpu.py: the stems' weight gradient ticked off before its
    tsr_reduce_splits is enqueued.  On one rank nothing would show; here the bucket is shipped holding the canary, the peer's
    share is overwritten by the late launch, and exactly the stem weights are reported -- on direct steps only (the first
    step copies finished tensors into the arena at its end)."""
    orig = _train.TrainEngine._stem_wgrad

    def early(self, c, gname, weight, x_coff, dz, dz_ctot, dz_coff, ns, grads):
        return orig(self, c, gname, weight, x_coff, dz, dz_ctot, dz_coff, ns, _EarlyPut(grads))

    case = tsr_case(1, 1, 1, "fp16x3")
    for seed in (BP.A, BP.B, BP.PEER):
        BP.plain(case, seed)                                   # the references: from the engine as it is
    monkeypatch.setattr(_train.TrainEngine, "_stem_wgrad", early)
    rig, fails = BP.run_sequence(case, monkeypatch, n_buckets=BP.PER_TENSOR)
    stems = {"input_layer_force.1.weight", "inputLayer_pattern_list.0.1.weight"}
    assert BP.failed(fails) == {"complete_when_shipped", "untouched_after_ship", "grad_is_the_mean"}, fails
    assert {d for _, d in fails} == stems and not [c for c, _ in fails if c.startswith("first:")], fails


# ---------------------------------------------------------------------------------------------------------- architecture
@pytest.mark.parametrize("T,Mb,R", [(2, 2, 1), (3, 1, 2)])
def test_more_frames_and_blocks(monkeypatch, T, Mb, R):
    rig = _run(tsr_case(T, Mb, R, "fp16x3"), monkeypatch, long=(T, Mb, R) == (2, 2, 1))
    assert len(rig.engine.arena.buckets) == len(FZ.param_names(T, Mb, R))


# ---------------------------------------------------------------------------------------------------------- bucket count
@pytest.mark.parametrize("n_buckets", [1, 3, 8, 1000])
def test_bucket_counts(monkeypatch, n_buckets):
    """1000 is more than there are tensors.  A bucket is closed once it holds total / n_buckets elements, so small tensors share
    one and a large tensor fills several buckets' worth: the count is at most n_buckets, and at least 2 as soon as n_buckets is
    (the last tensor, a stem weight of 1728 elements, is far smaller than half of the rest); with 1000 each of the ten
    convolutions of 16 k elements and more closes a bucket of its own."""
    rig = _run(tsr_case(1, 1, 1, "fp16x3"), monkeypatch, n_buckets=n_buckets)
    arena = rig.engine.arena
    assert not BP.layout_failures(arena, n_buckets)          # (which bounds the count by min(n_buckets, tensors))
    nb = len(arena.buckets)
    assert nb == 1 if n_buckets == 1 else nb >= (10 if n_buckets == 1000 else 2)


# ----------------------------------------------------------------------------------------------------------- frozen sets
FROZEN = [(pat, T, "fp16x3") for pat in FZ.PATTERNS for T in (1, 2)] + [("trunk", 1, "bf16")]


def _frozen_case(pattern, T, impl):
    if impl == "bf16":          # the bf16 case of tests/test_gpu_frozen.py keeps its own size
        return tsr_case(T, 2, 1, impl, pattern=pattern, sf=10, B=4)
    return tsr_case(T, 3, 1, impl, pattern=pattern)


@pytest.mark.parametrize("pattern,T,impl", FROZEN, ids=[f"{p}-T{T}-{i}" for p, T, i in FROZEN])
def test_frozen_sets(monkeypatch, pattern, T, impl):
    case = _frozen_case(pattern, T, impl)
    rig = _run(case, monkeypatch, long=impl == "bf16")
    want = case.want(rig.module)
    if not want:          # all_frozen_dx: the taxels ask for a gradient, nothing else does -- no arena, nothing on the wire
        assert case.dx and rig.engine.arena is None and all(m == ["first"] for _, m in rig.steps)
        return
    plan = _train.backward_plan(T, len(rig.module.patternFeatureExtra_layer), 1, want, case.dx)
    assert rig.engine.arena.names == FZ.production_order(plan, want)


def test_a_changed_freeze_pattern_lays_the_arena_out_again(monkeypatch):
    """The want-set changes between two steps: the next backward takes the first path again (nothing leaves from inside it),
    the one after it is direct on the new layout.  Then the set grows again in front of a twice-applied graph."""
    all_, trunk = tsr_case(1, 3, 1, "fp16x3", pattern="all"), tsr_case(1, 3, 1, "fp16x3", pattern="trunk")
    rig = BP.Rig(all_, monkeypatch, BP.PER_TENSOR)
    fails = rig.step("first", [BP.A], BP.PEER) + rig.step("direct", [BP.A], BP.PEER)
    old = rig.engine.arena
    rig.switch(trunk)
    fails += rig.step("first", [BP.A], BP.PEER)
    new = rig.engine.arena
    assert new is not old and rig.sync.arena is new and set(new.names) == set(trunk.want(rig.module)) < set(old.names)
    fails += rig.step("direct", [BP.A], BP.PEER) + rig.step("direct", [BP.B], BP.A)
    assert rig.engine.arena is new
    # every parameter trains again and the very next graph applies the model twice: that backward drops the arena but may not
    # lay a new one out, so finish() must reduce the summed .grad tensors themselves (bound to the old layout it left the
    # trunk's gradients rank-local); the step after it lays the full arena out
    rig.switch(all_)
    fails += rig.step("flat", [BP.A, BP.B], BP.PEER) + rig.step("first", [BP.A], BP.PEER) + rig.step("direct", [BP.B], BP.PEER)
    assert not fails, fails
    assert rig.engine.arena.names == old.names


# -------------------------------------------------------------------------------------------------------- held BatchNorm
@pytest.mark.parametrize("impl", ["fp16x3", "f32"])
@pytest.mark.parametrize("held", ["none", "all", "seqs", "mixed", "stem"])
def test_held_batchnorm(monkeypatch, held, impl):
    """BatchNorm layers in eval mode inside the training module: dgamma / dbeta come from tsr_bn_bwd_finalize_eval, the mixed
    stage-1 pair from the shared finalize; "seqs" also freezes the trunk, so held layers there produce no gradient at all."""
    case = tsr_case(2, 1, 1, impl, held=held)
    rig = _run(case, monkeypatch)
    assert {n for n, mod in rig.module.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and not mod.training} == \
        set(BM.pattern_paths(rig.module, held))


# -------------------------------------------------------------------------------------------------------- taxel gradient
@pytest.mark.parametrize("dx", [False, True], ids=["no_dx", "dx"])
def test_taxel_gradient_on_and_off(monkeypatch, dx):
    """With ``LR.requires_grad_()`` the stem_dgrad launches run between the stems' weight gradients; the taxel gradient of every
    backward is the plain one bit for bit (``input_grad``)."""
    _run(tsr_case(2, 2, 1, "fp16x3", dx=dx), monkeypatch)


# ----------------------------------------------------------------------------------------------------- standalone blocks
@pytest.mark.parametrize("impl", BC.IMPLS)
@pytest.mark.parametrize("kind", BC.KINDS)
def test_standalone_blocks(monkeypatch, kind, impl):
    rig = _run(block_case(kind, impl), monkeypatch, long=(kind, impl) == ("msrb", "fp16x3"))
    copies = {n for c, n in rig.sink_calls[1][1] if c == "put_copy"}
    assert copies == (_stage1_bn() if kind == "msrb" else set())


@pytest.mark.parametrize("kind,frozen,x_grad", FZ.BLOCK_SUBSETS, ids=[f"{k}-{f[0]}-x{int(x)}" for k, f, x in FZ.BLOCK_SUBSETS])
def test_standalone_blocks_with_frozen_parameters(monkeypatch, kind, frozen, x_grad):
    case = block_case(kind, "fp16x3", frozen, x_grad)
    rig = _run(case, monkeypatch)
    want = case.want(rig.module)
    assert rig.engine.arena.names == FZ.production_order(_train.block_backward_plan(kind, want, x_grad), want)
