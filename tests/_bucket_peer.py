"""A simulated second rank inside one process, for the in-backward gradient buckets of tactilesr_amd.ddp (used by
tests/test_bucket_peer_cpu.py on toy engines and by tests/test_gpu_bucket_completeness.py and tests/test_gpu_frozen.py on the
HIP engines).  Host only: nothing here needs a GPU, a process group or a second process.

``GradSync`` ships a bucket the moment its last gradient is ``put``.  On one rank the all-reduce is the identity, so a bucket
shipped before its slots were final still ends with the right contents.  Here ``dist.all_reduce`` is replaced by a function that
ADDS A PEER'S VALUES to exactly the range it is handed, at call time, on the current stream -- what the wire does to the buffer.
A slot written after that loses the peer's share; a slot not yet written has the share added to whatever lay there.

* ``SinkLog``        wraps ``ddp.GradSink``: the mode of every backward and each ``dest`` / ``put`` / ``put_copy`` it made.
* ``FakeAllReduce``  the peer: maps the tensor to peer values by its offset into ``arena.flat`` (or, in the ``finish_flat``
                     path, by ``module.parameters()`` order), keeps a copy of what the range held when it was shipped, records
                     ``(bucket | "flat", call index)``; its work objects stay pending until ``wait()``.
* ``Case``           how to build a fresh model of one configuration, its seeded batches and its loss; ``plain`` = the gradient
                     of one batch on a fresh model without ``GradSync`` (what another rank would hold).
* ``Rig``            one model under a ``GradSync`` with ``world = 2`` and the fake peer; ``step`` runs one step of a given kind
                     and returns the list of failed checks as ``(check name, detail)``.
* ``run_sequence``   first, direct, direct on a new batch -- and the long sequence.

Expected values are ``(local + peer) / 2`` computed on the device with the two operations the simulated path performs, so
the comparison is ``torch.equal``.  Before every backward that takes the direct path the arena is filled with NaN.

The checks, by name (``CHECKS``):
  arena_is_the_want_set, every_wanted_put, put_once, only_wanted_put, no_dest_after_put, mode,
  buckets_in_order_inside_backward, nothing_shipped_inside_backward, complete_when_shipped, untouched_after_ship,
  grad_is_the_mean, grad_aliases_slot, frozen_have_no_grad, no_nan, works_waited, input_grad, second_backward_refused
"""
from collections import Counter

import torch

from tactilesr_amd import ddp

CHECKS = ("arena_is_the_want_set", "every_wanted_put", "put_once", "only_wanted_put", "no_dest_after_put", "mode",
          "buckets_in_order_inside_backward", "nothing_shipped_inside_backward", "complete_when_shipped",
          "untouched_after_ship", "grad_is_the_mean", "grad_aliases_slot", "frozen_have_no_grad", "no_nan", "works_waited",
          "input_grad", "second_backward_refused")
PER_TENSOR = 1 << 30          # engine.n_buckets that gives every tensor its own bucket: each `put` ships at once


# ------------------------------------------------------------------------------------------------------ the sink recorder
def sink_mode(sink):
    return "first" if sink.first else "direct" if sink.direct else "shared" if sink.shared else "accum"


class SinkLog:
    """While active, every ``ddp.GradSink`` is a logging subclass: ``modes`` is the case each backward took (first / direct /
    accum / shared), ``backwards`` one ``(mode, [(call, name), ...])`` per backward with call in dest / put / put_copy
    (the ``dest`` and ``put`` inside a ``put_copy`` are not listed again)."""

    def __enter__(self):
        self.modes = modes = []
        self.backwards = backwards = []
        self._orig = orig = ddp.GradSink

        class Logged(orig):
            def __init__(self, *a, **kw):
                self._calls, self._quiet = [], False
                super().__init__(*a, **kw)
                modes.append(sink_mode(self))
                backwards.append((modes[-1], self._calls))

            def dest(self, name, shape):
                if not self._quiet:
                    self._calls.append(("dest", name))
                return super().dest(name, shape)

            def put(self, name, t):
                if not self._quiet:
                    self._calls.append(("put", name))
                return super().put(name, t)

            def put_copy(self, name, src):
                self._calls.append(("put_copy", name))
                self._quiet = True
                try:
                    return super().put_copy(name, src)
                finally:
                    self._quiet = False
        ddp.GradSink = Logged
        return self

    def __exit__(self, *exc):
        ddp.GradSink = self._orig
        return False


# ------------------------------------------------------------------------------------------------------------ the peer
class _Work:
    def __init__(self):
        self.waited = False

    def wait(self):
        self.waited = True
        return True


class FakeAllReduce:
    """Stands in for ``dist.all_reduce`` (SUM over two ranks): t += the peer's values of exactly t's range, now."""

    def __init__(self, sync):
        self.sync = sync
        self.peer = {}               # name -> the peer's gradient of the step being run
        self.calls = []              # (bucket index | "flat" | "?", call index)
        self.shipped = {}            # bucket index | "flat" -> what the range held when it was handed over
        self.works = []
        self._flat_for = None        # the arena the cached arena-shaped buffer of peer values was built for (per step)
        self._flat = None

    def begin_step(self, peer):
        self.peer = peer
        self.calls, self.shipped, self.works = [], {}, []
        self._flat_for = self._flat = None

    def _peer_flat(self, arena):
        if self._flat_for is not arena:
            flat = torch.zeros_like(arena.flat)
            for n in arena.names:
                flat[arena.offsets[n]:arena.offsets[n] + arena.shapes[n].numel()] = self.peer[n].reshape(-1)
            self._flat_for, self._flat = arena, flat
        return self._flat

    def __call__(self, t, op=None, group=None, async_op=False):
        assert op is None or op == ddp.dist.ReduceOp.SUM
        arena = self.sync.arena          # (the GradSync's: every call comes from its bucket callback or its finish())
        if arena is not None and t.untyped_storage().data_ptr() == arena.flat.untyped_storage().data_ptr():
            a = t.storage_offset() - arena.flat.storage_offset()
            b = a + t.numel()
            assert t.is_contiguous() and 0 <= a and b <= arena.flat.numel()
            key = arena.buckets.index((a, b)) if (a, b) in arena.buckets else "?"
            self.shipped[key] = t.detach().clone()
            t.add_(self._peer_flat(arena)[a:b])
        else:
            named = dict(self.sync.module.named_parameters())
            names = [n for n, p in named.items() if p.requires_grad and p.grad is not None]
            peer = torch.cat([self.peer[n].reshape(-1) for n in names]) if names else t.new_zeros(0)
            assert t.dim() == 1 and t.numel() == peer.numel(), (t.shape, peer.numel())
            key = "flat"
            self.shipped[key] = t.detach().clone()
            t.add_(peer)
        self.calls.append((key, len(self.calls)))
        if not async_op:
            return None
        self.works.append(_Work())
        return self.works[-1]


def make_sync(module, engine):
    """A ``GradSync`` without a process group (world 1), told it has a peer: ``_check_layout`` returns early without a group."""
    assert not ddp.dist.is_initialized()
    sync = ddp.GradSync(module, engine=engine)
    assert sync.world == 1 and engine.grad_sync is sync
    sync.world = 2
    return sync


# ------------------------------------------------------------------------------------------------------------ the cases
class Case:
    """One configuration.  ``build()`` -> a fresh module in the seeded state (device, modes and ``requires_grad`` flags set);
    ``engine(module)`` -> its backward engine; ``batch(seed)`` -> fresh input tensors (a taxel tensor that wants a gradient is
    a new leaf each time, first in the tuple); ``loss(module, batch)`` -> scalar; ``flags(module)`` re-applies the
    ``requires_grad`` flags and modes of this case to a module built for another one of the same architecture."""

    def __init__(self, key, build, engine, batch, loss, flags=None, dx=False):
        self.key, self.build, self.engine, self.batch, self.loss = key, build, engine, batch, loss
        self.flags = flags if flags is not None else (lambda module: None)
        self.dx = dx

    def want(self, module):
        return frozenset(n for n, p in module.named_parameters() if p.requires_grad)


_PLAIN = {}          # (case key, seed) -> (grads, dx); only the entries of the most recent case key are kept


def plain(case, seed):
    """The gradient of batch `seed` on a fresh model without GradSync: ({name: grad}, input gradient or None)."""
    if _PLAIN and next(iter(_PLAIN))[0] != case.key:
        _PLAIN.clear()
    if (case.key, seed) not in _PLAIN:
        m = case.build()
        assert getattr(case.engine(m), "grad_sync", None) is None
        b = case.batch(seed)
        case.loss(m, b).backward()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        assert set(grads) == set(case.want(m)), sorted(set(grads) ^ set(case.want(m)))[:4]
        dx = b[0].grad.detach().clone() if case.dx else None
        _PLAIN[(case.key, seed)] = (grads, dx)
    return _PLAIN[(case.key, seed)]


def mean2(local, peer):
    """What the simulated path leaves: the sum of two ranks, then the division by the world size."""
    return torch.add(local, peer).div_(2)


# -------------------------------------------------------------------------------------------------------------- the rig
class Rig:
    def __init__(self, case, monkeypatch, n_buckets=None):
        self.case = case
        self.module = case.build()
        self.engine = case.engine(self.module)
        if n_buckets is not None:
            self.engine.n_buckets = n_buckets
        self.sync = make_sync(self.module, self.engine)
        self.fake = FakeAllReduce(self.sync)
        monkeypatch.setattr(ddp.dist, "all_reduce", self.fake)          # restored by pytest after the test
        self.steps = []              # (kind, modes) of every step run: the tests count them
        self.sink_calls = []         # SinkLog.backwards of every backward, in order

    # ---- pieces
    def named(self):
        return dict(self.module.named_parameters())

    def want(self):
        return self.case.want(self.module)

    def switch(self, case):
        """Another freeze pattern / mode pattern on the same module."""
        case.flags(self.module)
        self.case = case

    def _zero(self):
        for p in self.module.parameters():
            p.grad = None

    def _canary(self):
        if self.engine.arena is not None:
            self.engine.arena.flat.fill_(float("nan"))

    def _backward(self, seeds, fails, expect_mode, ship):
        """One graph over the batches `seeds` (more than one: the model applied once per batch), one backward."""
        batches = [self.case.batch(s) for s in seeds]
        loss = sum(self.case.loss(self.module, b) for b in batches)
        n0 = len(self.fake.calls)
        with SinkLog() as log:
            loss.backward()
        inside = self.fake.calls[n0:]
        want = self.want()
        expect = [expect_mode if want else "first"] * len(seeds)          # (nothing to train: no arena is ever laid out)
        if log.modes != expect:
            fails.append(("mode", f"{log.modes} != {expect}"))
        for mode, calls in log.backwards:
            puts = Counter(n for c, n in calls if c in ("put", "put_copy"))
            missing = sorted(n for n in want if puts[n] == 0)
            twice = sorted(n for n, k in puts.items() if k > 1)
            other = sorted(n for n in puts if n not in want)
            if missing:
                fails.append(("every_wanted_put", f"never put: {missing[:4]}"))
            if twice:
                fails.append(("put_once", f"put more than once: {twice[:4]}"))
            if other:
                fails.append(("only_wanted_put", f"put but not wanted: {other[:4]}"))
            done = set()
            for c, n in calls:
                if c == "dest" and n in done:
                    fails.append(("no_dest_after_put", n))
                if c != "dest":
                    done.add(n)
        arena = self.engine.arena
        if ship:
            nb = len(arena.buckets) if arena is not None else 0
            if inside != [(k, k) for k in range(nb)]:
                fails.append(("buckets_in_order_inside_backward", f"{inside[:6]} for {nb} buckets"))
        elif inside:
            fails.append(("nothing_shipped_inside_backward", f"{inside[:6]}"))
        for s, b in zip(seeds, batches):
            if self.case.dx:
                ref = plain(self.case, s)[1]
                if b[0].grad is None or not torch.equal(b[0].grad, ref):
                    fails.append(("input_grad", f"batch {s}"))
        self.steps[-1][1].extend(log.modes)
        self.sink_calls.extend(log.backwards)

    def _finish(self, fails, local, peer, direct, expect_arena=True):
        """``sync.finish()`` and everything that must hold after it; `local` is what this rank's gradient must be before the
        reduction (name -> tensor), `direct`: the buckets were shipped from inside backward."""
        fake, want = self.fake, self.want()
        n_inside = len(fake.calls)
        self.sync.finish()
        arena = self.engine.arena
        named = self.named()
        if any(not w.waited for w in fake.works) or self.sync._works:
            fails.append(("works_waited", "a work object was not waited for"))
        for n, p in named.items():
            if n not in want and p.grad is not None:
                fails.append(("frozen_have_no_grad", n))
        if arena is None:
            if want and expect_arena:
                fails.append(("arena_is_the_want_set", "no arena"))
        elif set(arena.names) != set(want):
            fails.append(("arena_is_the_want_set", f"{sorted(set(arena.names) ^ set(want))[:4]}"))
        if direct:
            if len(fake.calls) != n_inside:
                fails.append(("buckets_in_order_inside_backward", f"shipped late: {fake.calls[n_inside:][:4]}"))
        elif arena is not None and want:
            nb = len(arena.buckets)
            if sorted(k for k, _ in fake.calls) != list(range(nb)):
                fails.append(("nothing_shipped_inside_backward", f"finish() shipped {fake.calls[:6]} for {nb} buckets"))
        for n in sorted(want):
            p = named[n]
            exp = mean2(local[n], peer[n])
            if p.grad is None or not torch.equal(p.grad, exp):
                fails.append(("grad_is_the_mean", n))
            if arena is None or n not in arena.offsets:
                continue
            if p.grad is not None and p.grad.data_ptr() != arena.flat.data_ptr() + 4 * arena.offsets[n]:
                fails.append(("grad_aliases_slot", n))
            slot = arena.view(n)
            if bool(torch.isnan(slot).any()):
                fails.append(("no_nan", n))
            k = arena.bucket_of[n]
            if direct and k in fake.shipped:
                o = arena.offsets[n] - arena.buckets[k][0]
                was = fake.shipped[k][o:o + slot.numel()].view(slot.shape)
                if not torch.equal(was, local[n]):
                    fails.append(("complete_when_shipped", n))
                if not torch.equal(slot, mean2(was, peer[n])):
                    fails.append(("untouched_after_ship", n))
        return fails

    # ---- the steps
    def step(self, kind, seeds, peer_seed):
        """kind: first | direct | accum | no_sync | shared | flat (shared without an arena) | pending.  Returns the failed checks."""
        fails = []
        case, fake = self.case, self.fake
        peer = plain(case, peer_seed)[0]
        g = [plain(case, s)[0] for s in seeds]
        self.steps.append((kind, []))
        fake.begin_step(peer)
        if kind in ("first", "direct"):
            self._zero()
            if kind == "direct":
                self._canary()
            self._backward(seeds, fails, kind, ship=kind == "direct" and bool(self.want()))
            local = g[0]
        elif kind == "accum":
            prev = {n: p.grad.detach().clone() for n, p in self.named().items() if p.grad is not None}
            self._backward(seeds, fails, "accum", ship=False)
            local = {n: torch.add(prev[n], g[0][n]) for n in g[0]}
        elif kind == "no_sync":
            self._zero()
            self._canary()
            with self.sync.no_sync():
                self._backward(seeds[:1], fails, "direct", ship=False)
            self._backward(seeds[1:], fails, "accum", ship=False)
            local = {n: torch.add(g[0][n], g[1][n]) for n in g[0]}
        elif kind in ("shared", "flat"):
            self._zero()
            self._backward(seeds, fails, "shared", ship=False)
            local = {n: torch.add(g[0][n], g[1][n]) for n in g[0]}
        elif kind == "pending":
            self._zero()
            self._canary()
            self._backward(seeds[:1], fails, "direct", ship=True)
            shipped = list(fake.calls)
            try:
                case.loss(self.module, case.batch(seeds[1])).backward()
                fails.append(("second_backward_refused", "no error"))
            except RuntimeError as e:
                if "no_sync" not in str(e):
                    fails.append(("second_backward_refused", str(e)[:80]))
            if fake.calls != shipped:
                fails.append(("second_backward_refused", "the refused backward shipped something"))
            local = g[0]
        else:
            raise KeyError(kind)
        if kind == "flat":
            if self.engine.arena is not None or self.sync.arena is not None:
                fails.append(("mode", "an arena exists: finish_flat is not reached"))
            self._finish(fails, local, peer, direct=False, expect_arena=False)
            if fake.calls != [("flat", 0)]:
                fails.append(("nothing_shipped_inside_backward", f"finish_flat made the calls {fake.calls[:4]}"))
        else:
            self._finish(fails, local, peer, direct=kind in ("direct", "pending") and bool(self.want()))
        return [(f"{kind}: {c}", d) for c, d in fails]


def failed(fails):
    """The set of check names in a list of failures."""
    return {c.split(": ", 1)[1] for c, _ in fails}


A, B, PEER = 11, 12, 13          # the seeds of the two own batches and of the peer's


def run_sequence(case, monkeypatch, long=False, n_buckets=None):
    """first, direct, direct on a new batch; `long` adds accumulation, no_sync micro-batches, the model applied twice in one
    graph (with an arena, and on a fresh model without one), a plain direct step and the refused second backward: eleven
    backward calls in all.  Returns (rig, failures)."""
    rig = Rig(case, monkeypatch, n_buckets)
    fails = rig.step("first", [A], PEER)
    fails += rig.step("direct", [A], PEER)
    fails += rig.step("direct", [B], A)
    if long:
        fails += rig.step("accum", [A], PEER)
        fails += rig.step("no_sync", [A, B], PEER)
        fails += rig.step("shared", [A, B], PEER)
        fresh = Rig(case, monkeypatch, n_buckets)
        fails += fresh.step("flat", [B, A], PEER)
        monkeypatch.setattr(ddp.dist, "all_reduce", rig.fake)
        fails += rig.step("direct", [B], PEER)
        fails += rig.step("pending", [A, B], B)
        rig.steps += fresh.steps
    return rig, fails


def layout_failures(arena, n_buckets):
    """The buckets tile [0, total) at tensor boundaries and every slot starts on a 256-byte boundary."""
    out = []
    bounds = {arena.offsets[n] for n in arena.names} | {arena.total}
    b = arena.buckets
    if not (b[0][0] == 0 and b[-1][1] == arena.total and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1))):
        out.append(f"buckets do not tile [0, {arena.total}): {b[:4]}")
    if any(lo not in bounds or hi not in bounds or lo >= hi for lo, hi in b):
        out.append("a bucket is empty or is cut inside a tensor")
    if not 1 <= len(b) <= min(n_buckets, len(arena.names)):
        out.append(f"{len(b)} buckets for n_buckets = {n_buckets}, {len(arena.names)} tensors")
    base = arena.flat.data_ptr() if arena.flat.is_cuda else 0          # (the host allocator promises 64 bytes only)
    for n in arena.names:
        if (base + 4 * arena.offsets[n]) % 256:
            out.append(f"{n} does not start on a 256-byte boundary")
        lo, hi = b[arena.bucket_of[n]]
        if not (lo <= arena.offsets[n] and arena.offsets[n] + arena.shapes[n].numel() <= hi):
            out.append(f"{n} is not inside its bucket")
    if [arena.bucket_of[n] for n in arena.names] != sorted(arena.bucket_of[n] for n in arena.names):
        out.append("bucket numbers do not follow production order")
    return out
