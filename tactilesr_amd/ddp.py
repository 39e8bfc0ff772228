"""Data-parallel training over the GPUs of one node: one process per GPU, weights replicated, batch sharded by
sample, rank-local BatchNorm statistics (what torch DDP without SyncBN does -- SURVEY.md section 5), and ONE
collective per step: the all-reduce (mean) of the 18.33 MB fp32 gradient over RCCL/xGMI, cut into buckets that are
issued FROM INSIDE backward as soon as their last gradient is final, so they run under the remaining backward
kernels.  The reference only carries the latent hooks for this (cpu/distributed.py:171-217, cpu/trainer.py:172-176);
no script wires it, so this is the build's own design.

Pieces
* ``GradArena`` -- one flat fp32 buffer holding every parameter gradient, laid out in the ORDER BACKWARD PRODUCES
  THEM, cut into contiguous buckets.  The backward engine writes each weight gradient straight into its arena view
  (``tsr_reduce_splits`` writes there: no copy in, no copy out) and ticks it off; when a bucket's last tensor is
  ticked the arena fires ``on_bucket_ready``.  The arena is engine-agnostic (the CPU tests drive it from a toy
  autograd function).
* ``GradSync`` -- owns the process group side: on ``bucket_ready`` it enqueues ``all_reduce(bucket, async_op=True)``
  (RCCL orders it after the producing kernels through the stream it was called on, then runs it on its own stream),
  ``finish()`` (between ``backward()`` and ``optimizer.step()``) waits for the works, turns sums into means and
  makes every ``p.grad`` the arena view.  ``broadcast_parameters`` sends ALL parameters and ALL buffers (BatchNorm
  running statistics included) from one rank.

On a full-mesh xGMI node 18 MB moves in well under 1 ms against >100 ms of backward compute: bucket granularity only
decides how early the first byte leaves, not the step time.
"""
from __future__ import annotations

import weakref
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

_ALIGN = 64          # arena views start on 256-B boundaries (16-B vector accesses in the fused Adam kernel)


def init_distributed(backend: str = "nccl"):
    """env:// rendezvous, one process per GPU (torchrun sets RANK / LOCAL_RANK / WORLD_SIZE).
    backend "nccl" is RCCL on ROCm; "gloo" is used by the CPU tests."""
    import os
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if backend == "nccl":
        local = local % torch.cuda.device_count()
        torch.cuda.set_device(local)
        dist.init_process_group(backend="nccl", init_method="env://", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend=backend, init_method="env://")
    return rank, world, local


def shard_batch(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous sample range of this rank (global batch split B/world per GPU)."""
    per = (n + world - 1) // world
    return min(n, rank * per), min(n, (rank + 1) * per)


def equal_shard(n: int, rank: int, world: int) -> List[int]:
    """Sample indices of this rank when EVERY rank must see the same count (a data-parallel epoch: a rank with fewer
    batches would leave the others blocked in their all-reduce).  ceil(n/world) per rank; the tail wraps around to the
    head of the set, like torch's DistributedSampler pads."""
    per = (n + world - 1) // world
    return [(rank * per + i) % n for i in range(per)] if n > 0 else []


class GradArena:
    """Flat gradient buffer in backward-production order, with bucket completion tracking."""

    def __init__(self, layout: Sequence[Tuple[str, torch.Size]], device, n_buckets: int = 8):
        self.names = [n for n, _ in layout]
        self.shapes: Dict[str, torch.Size] = {n: torch.Size(s) for n, s in layout}
        self.offsets: Dict[str, int] = {}
        off = 0
        for n, s in layout:
            self.offsets[n] = off
            off += (torch.Size(s).numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.total = off
        self.flat = torch.zeros(max(off, 1), dtype=torch.float32, device=device)
        # contiguous buckets of ~equal size, cut at tensor boundaries
        target = max(1, self.total // max(1, n_buckets))
        self.buckets: List[Tuple[int, int]] = []
        self.bucket_of: Dict[str, int] = {}
        start = 0
        for i, n in enumerate(self.names):
            self.bucket_of[n] = len(self.buckets)
            end = self.offsets[self.names[i + 1]] if i + 1 < len(self.names) else self.total
            if end - start >= target and len(self.buckets) < n_buckets - 1 and i + 1 < len(self.names):
                self.buckets.append((start, end))
                start = end
        self.buckets.append((start, self.total))
        self._members = [sum(1 for n in self.names if self.bucket_of[n] == k) for k in range(len(self.buckets))]
        self._left = list(self._members)
        self.on_bucket_ready: Optional[Callable[[int, torch.Tensor], None]] = None

    def view(self, name: str) -> torch.Tensor:
        """A FRESH view object of `name`'s slot (autograd may adopt it as .grad without a copy)."""
        o = self.offsets[name]
        return self.flat[o:o + self.shapes[name].numel()].view(self.shapes[name])

    def begin(self) -> None:
        self._left = list(self._members)

    def done(self, name: str) -> None:
        """`name`'s slot holds its final value; fires the bucket callback when its bucket is complete."""
        k = self.bucket_of[name]
        self._left[k] -= 1
        if self._left[k] == 0 and self.on_bucket_ready is not None:
            a, b = self.buckets[k]
            self.on_bucket_ready(k, self.flat[a:b])

    def bucket(self, k: int) -> torch.Tensor:
        a, b = self.buckets[k]
        return self.flat[a:b]


def note_forward(owner, token) -> None:
    """An autograd forward of engine ``owner`` that WILL be differentiated registers its context object here (weakly:
    a graph that is dropped without a backward un-registers itself).  ``GradSink`` reads the set to find out whether
    the backward it serves is the only outstanding application of the engine -- see its ``shared`` case."""
    live = getattr(owner, "_live_forwards", None)
    if live is None:
        live = owner._live_forwards = weakref.WeakSet()
    live.add(token)


class GradSink:
    """What a backward engine writes its parameter gradients through (one per backward call).

    ``owner`` is the engine: it carries ``arena`` (None until the first backward has revealed the production order),
    ``grad_sync`` (None on one GPU) and ``n_buckets``.  ``want`` (optional) names the parameters this backward produces
    a gradient for -- the trainable ones; frozen parameters have no arena slot, and a stale ``.grad`` one of them still
    carries does not count below.  An arena laid out for another want-set is dropped like one laid out for another
    module tree: this backward takes the ``first`` path again (the GradSync is re-bound, the fused Adam builds one new
    chunk table).  Without ``want`` every parameter of ``named_params`` counts.  The cases:
      direct  -- the arena exists and every wanted parameter's .grad is None (``zero_grad()``'s default): ``dest`` hands out
                 arena views, ``put`` ticks the arena, complete buckets go to the wire from inside backward;
      first   -- no arena yet: gradients land in fresh tensors while the order is recorded; ``finalize`` builds the
                 arena in that order, moves them in and binds the GradSync (buckets are reduced in ``finish``);
      accum   -- some .grad is set (gradient accumulation, ``zero_grad(set_to_none=False)``): fresh tensors are
                 returned so autograd can add them to the existing .grad; nothing is issued early;
      shared  -- the engine was applied MORE THAN ONCE inside the graph being differentiated (``f(m(a)) + f(m(b))``, a
                 shared block called twice): autograd sums the per-application gradients only AFTER all of them have
                 run, so none of them may own the arena slots (the second would overwrite the first's views before the
                 sum).  ``token`` is the context object the forward registered with ``note_forward``; a backward whose
                 token is not the only live one -- and every later backward of that graph, down to the one that finds
                 itself alone again -- returns fresh tensors like ``accum``; ``GradSync.finish`` then reduces the summed
                 ``.grad`` tensors.
    """

    def __init__(self, owner, named_params: Dict[str, torch.nn.Parameter], device, token=None, want=None):
        self.owner, self.device = owner, device
        arena = laid_out = getattr(owner, "arena", None)
        if arena is not None and any(n not in named_params or named_params[n].shape != arena.shapes[n]
                                     for n in arena.names):
            arena = owner.arena = None                                   # the module tree changed: lay out again
        if arena is not None and want and set(arena.names) != set(want):
            arena = owner.arena = None                                   # another set of parameters trains: lay out again
        counted = named_params.values() if want is None else [named_params[n] for n in want if n in named_params]
        live = getattr(owner, "_live_forwards", None)
        alone = True
        if live is not None:
            alone = not any(t is not token for t in live)
            if token is not None:
                live.discard(token)
        self.shared = bool(getattr(owner, "_shared_graph", False)) or not alone
        owner._shared_graph = self.shared and not alone                  # the graph's last backward clears the mark
        self.first = arena is None and not self.shared
        self.direct = (arena is not None and not self.shared
                       and all(p.grad is None for p in counted))
        self.arena = arena if self.direct else None
        sync = getattr(owner, "grad_sync", None)
        if sync is not None:
            sync.backward_started("first" if self.first else ("direct" if self.direct else
                                                              ("shared" if self.shared else "accum")), device)
            if arena is None and laid_out is not None and sync.arena is laid_out:
                # the layout was dropped above and this backward may not lay a new one out (shared): a GradSync still bound
                # to the old arena would reduce the old names only -- unbound, finish() reduces the .grad tensors themselves
                sync.arena = None
        if self.direct:
            arena.begin()
        self.out: Dict[str, torch.Tensor] = {}
        self.order: List[Tuple[str, torch.Size]] = []

    def dest(self, name: str, shape) -> torch.Tensor:
        if self.arena is not None:
            if name not in self.arena.offsets:
                raise KeyError(f"gradient '{name}' has no slot in the arena (laid out for a different module tree)")
            return self.arena.view(name)
        return torch.empty(torch.Size(shape), dtype=torch.float32, device=self.device)

    def put(self, name: str, t: torch.Tensor) -> None:
        self.out[name] = t
        self.order.append((name, t.shape))
        if self.arena is not None:
            self.arena.done(name)

    def put_copy(self, name: str, src: torch.Tensor) -> None:
        d = self.dest(name, src.shape)
        d.copy_(src)
        self.put(name, d)

    def finalize(self) -> Dict[str, torch.Tensor]:
        if self.first and self.order:
            arena = GradArena(self.order, self.device, getattr(self.owner, "n_buckets", 8))
            for n, t in self.out.items():
                arena.view(n).copy_(t)
            self.out = {n: arena.view(n) for n in self.out}
            self.owner.arena = arena
            sync = getattr(self.owner, "grad_sync", None)
            if sync is not None:
                sync.bind(arena)
        return self.out


class GradSync:
    """Gradient averaging for a replicated model whose backward fills a ``GradArena``.

    Gradient accumulation over micro-batches: run every backward but the last under ``with sync.no_sync():`` (nothing is
    put on the wire; autograd accumulates in place into the arena views), then ``finish()`` after the last one.  A second
    backward while bucket all-reduces of an earlier one are in flight would add local gradients on top of partially
    reduced ones -- that raises instead of silently averaging the wrong thing.

    ``broadcast_buffers=True`` reproduces torch-DDP's default: before every forward (``pre_forward()``, called by
    ``train_one_iter``) rank 0's buffers -- the BatchNorm running statistics and counters -- are broadcast, so every
    rank evaluates / checkpoints with the same statistics; ``False`` (default) keeps them rank-local after the start-up
    broadcast, i.e. rank r's running statistics describe rank r's shards."""

    def __init__(self, module: torch.nn.Module, group=None, engine=None, broadcast_buffers: bool = False):
        self.module = module
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.arena: Optional[GradArena] = None
        self.broadcast_buffers = bool(broadcast_buffers)
        self._works: Dict[int, object] = {}
        self._defer = False
        self.events: List[Tuple[str, int]] = []      # ("enqueue", bucket) / ("finish", n): the tests read the order
        # timing of the last step (see stats()): where in backward each bucket left, how long finish() waited
        self._t0 = None
        self._ev0 = None
        self._enq: List[Tuple[int, float, object]] = []      # (bucket, host ms since backward start, device event | None)
        self._wait_host_ms = 0.0
        self._wait_ev = None
        self.buffer_broadcasts = 0
        if engine is None and hasattr(module, "train_engine"):
            engine = module.train_engine()           # tactilesr_amd.TactileSR: its HIP backward engine
        if engine is not None:
            engine.grad_sync = self
            if getattr(engine, "arena", None) is not None:
                self.bind(engine.arena)

    # ---- wiring ----------------------------------------------------------------------------------------------
    def bind(self, arena: GradArena) -> None:
        """Called by the backward engine once its arena exists (after the first backward, and again whenever the set
        of trainable parameters changed and the arena was laid out anew).  With more than one rank the layouts are
        compared first: ranks that froze different parameters would reduce different tensors into each other."""
        self._check_layout(arena)
        self.arena = arena
        arena.on_bucket_ready = self._bucket_ready

    _LAYOUT_SLOTS = 256

    def _check_layout(self, arena: GradArena) -> None:
        """One small all-gather of a fixed-size table of running 63-bit hashes over the arena's (name, offset) pairs --
        entry i covers the first i + 1 pairs, the last entry the whole layout -- so the first entry that differs
        between two ranks points at the first parameter whose slot differs."""
        ranks = dist.get_world_size(self.group) if dist.is_initialized() else 1      # (the group's own size: it is a collective)
        if self.world == 1 or ranks < 2:
            return
        import hashlib
        h = hashlib.blake2b(digest_size=8)
        table = []
        for n in arena.names:
            h.update(f"{n}@{arena.offsets[n]};".encode())
            table.append(int.from_bytes(h.digest(), "little") >> 1)
        h.update(f"total@{arena.total}".encode())
        whole = int.from_bytes(h.digest(), "little") >> 1
        k = self._LAYOUT_SLOTS
        table = (table[:k - 1] + [whole] * k)[:k - 1] + [whole]
        mine = torch.tensor(table, dtype=torch.int64, device=arena.flat.device)
        every = [torch.empty_like(mine) for _ in range(ranks)]
        dist.all_gather(every, mine, group=self.group)
        for r, other in enumerate(every):
            diff = (other != mine).nonzero()
            if diff.numel():
                i = int(diff[0])
                here = arena.names[i] if i < min(len(arena.names), k - 1) else "<end of the layout>"
                raise RuntimeError(
                    f"GradSync: the gradient arena of this rank differs from rank {r}'s from entry {i} on ('{here}' "
                    f"here): every rank must train (and freeze) the same parameters -- a mismatch would reduce "
                    f"different tensors into each other")

    def no_sync(self):
        """Context manager: backward passes inside it put nothing on the wire (micro-batches of an accumulated step)."""
        sync = self

        class _NoSync:
            def __enter__(self_):
                self_.prev, sync._defer = sync._defer, True

            def __exit__(self_, *exc):
                sync._defer = self_.prev
                return False
        return _NoSync()

    def backward_started(self, mode: str, device) -> None:
        """Called by the GradSink at the start of every backward (mode: first / direct / accum)."""
        if self._works:
            raise RuntimeError(
                "GradSync: a backward pass started while the bucket all-reduces of a previous backward are still in "
                "flight -- with gradient accumulation run every micro-batch but the last under `with sync.no_sync():` "
                "(or call finish() after each backward)")
        import time
        self._t0 = time.perf_counter()
        self._enq = []
        self._ev0 = None
        if torch.device(device).type == "cuda":
            self._ev0 = torch.cuda.Event(enable_timing=True)
            self._ev0.record()

    def _mark_enqueue(self, k: int, t: torch.Tensor) -> None:
        import time
        ev = None
        if t.is_cuda:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
        self._enq.append((k, (time.perf_counter() - self._t0) * 1e3 if self._t0 is not None else 0.0, ev))

    def _bucket_ready(self, k: int, flat_slice: torch.Tensor) -> None:
        if self.world == 1 or self._defer:
            return
        self.events.append(("enqueue", k))
        self._mark_enqueue(k, flat_slice)
        self._works[k] = dist.all_reduce(flat_slice, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    # ---- per step --------------------------------------------------------------------------------------------
    def pre_forward(self) -> None:
        """torch-DDP ``broadcast_buffers=True`` semantics: rank 0's buffers before every forward (3 coalesced
        broadcasts: floating-point buffers, integer counters)."""
        if self.world == 1 or not self.broadcast_buffers:
            return
        with torch.no_grad():
            bufs = list(self.module.buffers())
            for kind in (True, False):
                ts = [b for b in bufs if b.is_floating_point() == kind]
                if not ts:
                    continue
                flat = torch.cat([t.reshape(-1).to(ts[0].dtype) for t in ts])
                dist.broadcast(flat, 0, group=self.group)
                off = 0
                for t in ts:
                    t.copy_(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()
        self.buffer_broadcasts += 1
        from . import _lib
        _lib.bump_param_epoch()       # eval-mode weight packs fold the running statistics

    def finish(self) -> None:
        """grad <- mean over ranks.  Call between backward() and optimizer.step().  Buckets that were not issued
        from inside backward (first step: the arena is built at its end; gradients accumulated over micro-batches
        under no_sync(); gradients accumulated into foreign tensors) are reduced here."""
        if self.world == 1:
            return
        if self._defer:
            raise RuntimeError("GradSync.finish() inside no_sync(): leave the context before the last micro-batch")
        if self.arena is None:
            # no backward has laid the arena out yet (every one so far served a graph that applies the engine more than
            # once): reduce the gradient tensors autograd summed, as one flat buffer
            gs = [p.grad for p in self.module.parameters() if p.requires_grad and p.grad is not None]
            if gs:
                flat = torch.cat([g.reshape(-1) for g in gs])
                dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
                flat.div_(self.world)
                off = 0
                for g in gs:
                    g.copy_(flat[off:off + g.numel()].view_as(g))
                    off += g.numel()
            self.events.append(("finish_flat", len(gs)))
            return
        import time
        arena = self.arena
        named = dict(self.module.named_parameters())
        stale = [n for n in arena.names if n in named and named[n].grad is not None
                 and named[n].grad.data_ptr() != arena.flat.data_ptr() + 4 * arena.offsets[n]]
        if stale and not self._works:
            # gradients live outside the arena (accumulated into foreign tensors): bring them in, reduce everything
            for n in stale:
                arena.view(n).copy_(named[n].grad)
        for k in range(len(arena.buckets)):
            if k not in self._works:
                self.events.append(("enqueue_late", k))
                self._mark_enqueue(k, arena.flat)
                self._works[k] = dist.all_reduce(arena.bucket(k), op=dist.ReduceOp.SUM, group=self.group,
                                                 async_op=True)
        # exposed communication: how long the step waits here for collectives that did not finish under backward --
        # on the device (events around the stream-side waits: RCCL's wait() parks the compute stream, not the host) and
        # on the host (gloo: wait() blocks the caller)
        ev_a = ev_b = None
        if arena.flat.is_cuda:
            ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev_a.record()
        t_w = time.perf_counter()
        for k in sorted(self._works):
            self._works[k].wait()
        self._wait_host_ms = (time.perf_counter() - t_w) * 1e3
        if ev_a is not None:
            ev_b.record()
            self._wait_ev = (ev_a, ev_b)
        self._works.clear()
        arena.flat.div_(self.world)
        for n in arena.names:
            p = named.get(n)
            if p is not None and p.requires_grad:
                p.grad = arena.view(n)          # autograd may have cloned the view it was handed: re-point
        self.events.append(("finish", len(arena.buckets)))

    __call__ = finish

    def stats(self) -> Dict[str, object]:
        """Timing of the LAST step (synchronises the device to read its events): per bucket the offset from the start of
        backward at which its all-reduce was enqueued (host clock and device clock), and the time finish() waited for
        collectives (``comm_wait_ms``: device stall when the tensors are on a GPU, host stall otherwise)."""
        out: Dict[str, object] = {"world": self.world, "buckets": len(self.arena.buckets) if self.arena else 0,
                                  "broadcast_buffers": self.broadcast_buffers}
        dev_wait = None
        if self._wait_ev is not None:
            self._wait_ev[1].synchronize()
            dev_wait = self._wait_ev[0].elapsed_time(self._wait_ev[1])
        out["comm_wait_ms"] = round(dev_wait if dev_wait is not None else self._wait_host_ms, 4)
        out["comm_wait_host_ms"] = round(self._wait_host_ms, 4)
        enq = []
        for k, host_ms, ev in self._enq:
            d = None
            if ev is not None and self._ev0 is not None:
                ev.synchronize()
                d = round(self._ev0.elapsed_time(ev), 3)
            enq.append({"bucket": k, "host_ms": round(host_ms, 3), "device_ms": d})
        out["bucket_enqueue_offsets"] = enq
        return out

    # ---- start-up --------------------------------------------------------------------------------------------
    def broadcast_parameters(self, src: int = 0) -> None:
        """Every replica starts from rank `src`'s state: ALL parameters (frozen ones too) and ALL buffers
        (BatchNorm running_mean / running_var / num_batches_tracked)."""
        if self.world == 1:
            return
        with torch.no_grad():
            for t in list(self.module.parameters()) + list(self.module.buffers()):
                dist.broadcast(t.data, src, group=self.group)
        from . import _lib
        _lib.bump_param_epoch()       # cached weight packs of the HIP modules are stale now
