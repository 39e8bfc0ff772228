"""The simulated second rank of tests/_bucket_peer.py can fail: on a toy engine in the style of tests/test_ddp_cpu.py (three
linear pieces, gradients produced in reverse layer order through the real GradSink / GradArena / GradSync), one correct
engine passes every check of every step kind, and each of four wrong engines is flagged by the check named for it.  This is the
CPU proof that tests/test_gpu_bucket_completeness.py would notice a HIP engine that hands a bucket over too early."""
import pytest
import torch

import _bucket_peer as BP

FAULTS = {"put_before_last_write": "complete_when_shipped", "write_after_put": "untouched_after_ship",
          "never_put": "every_wanted_put", "put_twice": "put_once"}


class _ToyEngine:
    """Stands in for model/_train.py's TrainEngine.  `fault` names what it does wrong, always on layer l2."""

    def __init__(self, module, fault=None):
        self.m, self.fault = module, fault
        self.arena = None
        self.grad_sync = None
        self.n_buckets = 3

    def backward(self, x, dy, want, token):
        from tactilesr_amd.ddp import GradSink
        sink = GradSink(self, dict(self.m.named_parameters()), x.device, token=token, want=want)
        for name in ("l3", "l2", "l1"):
            lin = getattr(self.m, name)
            fault = self.fault if name == "l2" else None
            if f"{name}.weight" in want:
                gw = sink.dest(f"{name}.weight", lin.weight.shape)
                if fault == "put_before_last_write":
                    sink.put(f"{name}.weight", gw)
                    torch.matmul(dy.t(), x, out=gw)
                else:
                    torch.matmul(dy.t(), x, out=gw)
                    sink.put(f"{name}.weight", gw)
                if fault == "write_after_put":
                    gw.copy_(dy.t() @ x)                       # the same value once more: a write all the same
                if fault == "put_twice":
                    sink.put(f"{name}.weight", gw)
            if f"{name}.bias" in want and fault != "never_put":
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
    def __init__(self, fault=None):
        super().__init__()
        self.l1, self.l2, self.l3 = (torch.nn.Linear(40, 24) for _ in range(3))
        self._engine = _ToyEngine(self, fault)

    def train_engine(self):
        return self._engine

    def forward(self, x):
        named = list(self.named_parameters())
        return _ToyFn.apply(self._engine, [n for n, _ in named], x, *[p for _, p in named])


def _case(fault=None, frozen=()):
    """The toy under `fault`; its plain gradients come from the correct engine (what the peer, and this rank, really hold)."""
    def flags(m):
        for n, p in m.named_parameters():
            p.requires_grad_(n not in frozen)

    def build(f=fault):
        torch.manual_seed(3)
        m = _Toy(f)
        flags(m)
        return m

    def batch(seed):
        return (torch.randn(6, 40, generator=torch.Generator().manual_seed(seed)),)

    case = BP.Case(("toy", fault, tuple(frozen)), build, lambda m: m.train_engine(), batch,
                   lambda m, b: m(b[0]).pow(2).mean(), flags=flags)
    return case


def _run(fault, monkeypatch, long=False, n_buckets=BP.PER_TENSOR, frozen=()):
    good = _case(None, frozen)
    for seed in (BP.A, BP.B, BP.PEER):                     # the references: from the correct engine, under the case's key
        BP.plain(good, seed)
    bad = _case(fault, frozen)
    bad.key = good.key
    return BP.run_sequence(bad, monkeypatch, long=long, n_buckets=n_buckets)


@pytest.mark.parametrize("n_buckets", [1, 3, BP.PER_TENSOR])
def test_the_correct_engine_passes_every_check_of_the_long_sequence(monkeypatch, n_buckets):
    rig, fails = _run(None, monkeypatch, long=True, n_buckets=n_buckets)
    assert not fails, fails
    assert [k for k, _ in rig.steps] == ["first", "direct", "direct", "accum", "no_sync", "shared", "direct", "pending", "flat"]
    # eleven backward() calls: the two graphs that apply the model twice run two engine passes each, the refused one none
    assert [len(m) for _, m in rig.steps] == [1, 1, 1, 1, 2, 2, 1, 1, 2]
    arena = rig.engine.arena
    assert not BP.layout_failures(arena, n_buckets)
    assert len(arena.buckets) == {1: 1, 3: 3, BP.PER_TENSOR: 6}[n_buckets]


def test_the_correct_engine_with_a_frozen_layer(monkeypatch):
    rig, fails = _run(None, monkeypatch, long=True, frozen=("l2.weight", "l1.bias"))
    assert not fails, fails
    assert rig.engine.arena.names == ["l3.weight", "l3.bias", "l2.bias", "l1.weight"]


def test_unfreezing_before_a_twice_applied_graph_reduces_the_new_parameters_too(monkeypatch):
    """The want-set grows and the very next graph applies the model twice: that backward drops the engine's arena but cannot
    lay a new one out (shared mode), so the GradSync must let go of the old layout as well -- finish() then reduces the summed
    ``.grad`` tensors themselves.  Bound to the old arena it reduced only the old names: l2's gradients stayed rank-local."""
    some, every = _case(None, ("l2.weight", "l2.bias")), _case(None)
    rig = BP.Rig(some, monkeypatch, BP.PER_TENSOR)
    fails = rig.step("first", [BP.A], BP.PEER) + rig.step("direct", [BP.A], BP.PEER)
    assert "l2.weight" not in rig.sync.arena.names
    rig.switch(every)
    fails += rig.step("flat", [BP.A, BP.B], BP.PEER)
    fails += rig.step("first", [BP.A], BP.PEER) + rig.step("direct", [BP.B], BP.PEER)
    assert not fails, fails
    assert len(rig.sync.arena.names) == 6


@pytest.mark.parametrize("fault", list(FAULTS))
def test_each_wrong_engine_is_flagged_by_the_check_named_for_it(monkeypatch, fault):
    rig, fails = _run(fault, monkeypatch)
    names = BP.failed(fails)
    print(fault, sorted(fails))
    assert FAULTS[fault] in names, (fault, fails)
    assert names <= set(BP.CHECKS)
    # the first step of an early put is harmless (fresh tensors, copied into the arena at the end): only direct steps show it
    if fault in ("put_before_last_write", "write_after_put"):
        assert not [c for c, _ in fails if c.startswith("first:")], fails
        assert "grad_is_the_mean" in names          # and the result is wrong, not merely the order
    # nothing but the faulty layer's tensors is reported
    assert all("l2." in d for c, d in fails if c.split(": ")[1] in ("complete_when_shipped", "untouched_after_ship",
                                                                      "grad_is_the_mean", "no_nan"))


def test_an_early_put_in_the_middle_of_a_bucket_is_not_visible_and_per_tensor_buckets_make_it_so(monkeypatch):
    """Why the GPU cases run with one bucket per tensor: with three buckets l2.weight is not the last tensor of its bucket, so
    the bucket leaves after the late write and the result is right -- until a layout change moves the boundary."""
    _, fails = _run("put_before_last_write", monkeypatch, n_buckets=3)
    assert not fails, fails
    _, fails = _run("put_before_last_write", monkeypatch, n_buckets=BP.PER_TENSOR)
    assert "complete_when_shipped" in BP.failed(fails)


def test_sink_log_lists_every_call_once():
    torch.manual_seed(0)
    m = _Toy()
    with BP.SinkLog() as log:
        m(torch.randn(4, 40)).sum().backward()
    assert log.modes == ["first"]
    assert log.backwards[0][1] == [(c, f"{l}.{k}") for l in ("l3", "l2", "l1")
                                   for c, k in (("dest", "weight"), ("put", "weight"), ("put_copy", "bias"))]
    from tactilesr_amd import ddp
    assert ddp.GradSink.__name__ == "GradSink"          # restored


def test_the_fake_is_restored_and_adds_exactly_the_range_it_is_handed(monkeypatch):
    import torch.distributed as dist
    orig = dist.all_reduce
    with monkeypatch.context() as mp:
        rig = BP.Rig(_case(), mp, n_buckets=BP.PER_TENSOR)
        assert dist.all_reduce is rig.fake
        assert not rig.step("first", [BP.A], BP.PEER)
        arena = rig.engine.arena
        arena.flat.zero_()
        rig.fake.begin_step({n: torch.full(arena.shapes[n], float(i + 1)) for i, n in enumerate(arena.names)})
        assert rig.fake(arena.bucket(2)) is None and rig.fake(arena.bucket(4), async_op=True).waited is False
        assert rig.fake.calls == [(2, 0), (4, 1)]
        for i, n in enumerate(arena.names):
            assert torch.equal(arena.view(n), torch.full(arena.shapes[n], float(i + 1) if i in (2, 4) else 0.0)), n
        pad = arena.flat.clone()
        for n in arena.names:
            pad[arena.offsets[n]:arena.offsets[n] + arena.shapes[n].numel()] = 0
        assert not bool(pad.any())                          # the padding between slots got nothing
    assert dist.all_reduce is orig
