"""torch.optim.Adam-compatible optimizer whose step is ONE launch of the fused HIP kernel ``tsr_adam_l2_multi``
over all parameter tensors (L2-in-gradient weight decay, i.e. torch.optim.Adam, not AdamW -- reference
train/tactileSR_train.py:212: ``optim.Adam(model.parameters(), lr, weight_decay)``; stepped at cpu/trainer.py:361).

It subclasses ``torch.optim.Optimizer`` so ``param_groups`` / ``state_dict`` / lr schedulers
(``optim.lr_scheduler.StepLR``, the warm-up wrapper) work unchanged; the state keys (``step``, ``exp_avg``,
``exp_avg_sq``) are torch.optim.Adam's, so checkpoints interoperate (cpu/trainer.py:401-421).

Per step the host builds nothing: a device table of (param, grad, exp_avg, exp_avg_sq, n) records, one per <= 4096
elements, is cached per set of live (param, grad) addresses -- with the engine's gradient arena those are the same
every step -- and the kernel walks it.  Parameters without a gradient are skipped exactly like torch does (the
Seqs transplant leaves an optimizer holding discarded modules, train/tactileSRSeqs_train.py:74-77).

A captured step (``tactilesr_amd.train.graph.GraphedTrainStep``) goes through ``_captured_step`` /
``_replay_rows``: the same kernel body launched through ``tsr_adam_l2_multi_dev``, which reads lr and the bias
corrections from a device buffer that is rewritten on the host before every replay.

Gradient-norm clipping (the reference trainer's ``clip_grad_norm``, cpu/trainer.py:354-356): ``step_clipped(max_norm)``
is ``torch.nn.utils.clip_grad_norm_(<the parameters with a gradient>, max_norm); step()`` without a host sync -- one
``tsr_grad_norm_multi`` (two kernels) over a chunk table of every group's gradients writes {total_norm, clip_coef} to a
device array, then every (group, step) set runs ``tsr_adam_l2_multi_clip``, which scales the gradient by that
coefficient, writes it back (torch leaves ``p.grad`` clipped) and takes the plain step on it.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import call, ptr, stream, c_int as _I, c_float as _F, TactileSRHipError

CHUNK = 4096
GN_PARTIALS = 256     # tsr_grad_norm_multi: one double partial per workgroup of its first kernel
GN_LAUNCHES = 2       # kernels one tsr_grad_norm_multi call issues


class _Rec(ctypes.Structure):         # mirror of tsr_adam_chunk (include/tactilesr_hip.h)
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_int), ("reserved", ctypes.c_int)]


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = {}           # key (every address the table holds) -> (device table, n_chunks)
        self.launches = 0           # kernel launches issued so far (tests: one per step)
        self.table_builds = 0       # device tables built so far (steady state with the gradient arena: exactly one)

    def _table(self, items, build=True):
        key = tuple((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                    for p, g, st in items)
        hit = self._tables.get(key)
        if hit is not None:
            return hit
        if not build:
            raise TactileSRHipError("tactilesr_amd.optim.Adam: no chunk table for these (param, grad, state) addresses; "
                                    "building one during a graph capture would be a host-to-device copy -- run an eager "
                                    "step with the same gradients first")
        recs = []
        for p, g, st in items:
            n = p.numel()
            for off in range(0, n, CHUNK):
                b = 4 * off
                recs.append((p.data_ptr() + b, g.data_ptr() + b, st["exp_avg"].data_ptr() + b,
                             st["exp_avg_sq"].data_ptr() + b, min(CHUNK, n - off), 0))
        arr = (_Rec * len(recs))(*recs)
        host = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).clone()
        dev = host.to(items[0][0].device)
        if len(self._tables) > 8:
            self._tables.clear()
        # The key IS the table: every address a record holds (param, grad, exp_avg, exp_avg_sq of every tensor) is part
        # of it, so a hit is valid whatever lived at those addresses in between -- no tensor has to be kept alive for
        # it (holding the gradients here pinned up to nine stale gradient sets of a model whose gradients are fresh
        # autograd tensors every step).
        self._tables[key] = (dev, len(recs))
        self.table_builds += 1
        return self._tables[key]

    def _launch_sets(self, advance):
        """Yields (group, step, [(p, grad, state)]) in launch order: per group, the parameters with a gradient, split by
        their (1-based) step number.  ``advance`` increments ``state["step"]`` (the eager step, group by group as it
        launches); without it the step number is the one the next step will use and nothing is created or changed."""
        for group in self.param_groups:
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32:
                    raise TactileSRHipError("tactilesr_amd.optim.Adam needs fp32 parameters on a ROCm device")
                if not p.is_contiguous():
                    raise TactileSRHipError("tactilesr_amd.optim.Adam needs contiguous parameters")
                g = p.grad
                st = self.state[p]
                if advance:
                    if not g.is_contiguous():
                        g = p.grad = g.contiguous()
                    if len(st) == 0:
                        st["step"] = torch.tensor(0.0)
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["step"] += 1
                    step = int(st["step"].item())      # CPU scalar: no device sync
                else:
                    if len(st) == 0 or not g.is_contiguous():
                        raise TactileSRHipError("tactilesr_amd.optim.Adam: a captured step needs the optimizer state "
                                                "and contiguous gradients of an eager step first")
                    step = int(st["step"].item()) + 1
                by_step.setdefault(step, []).append((p, g, st))
            for step, items in by_step.items():
                yield group, step, items

    def _grad_norm(self, sets, max_norm, out, work, build=True):
        """Issue ``tsr_grad_norm_multi`` over the gradients of every (param, grad) item of ``sets`` (as
        ``_launch_sets`` yields them): out = {total_norm, clip_coef} (a device float32 tensor of >= 2 elements), work
        a device float64 tensor of >= GN_PARTIALS elements.  Returns the chunk table the launch reads."""
        if out.dtype != torch.float32 or out.numel() < 2 or work.dtype != torch.float64 or work.numel() < GN_PARTIALS:
            raise TactileSRHipError("gradient norm: out needs 2 float32 elements, work GN_PARTIALS float64 elements")
        dev, n_chunks = self._table([it for _, _, items in sets for it in items], build=build)
        call("tsr_grad_norm_multi", ptr(dev), _I(n_chunks), _F(max_norm), ptr(work), ptr(out), stream())
        return dev

    @torch.no_grad()
    def _captured_grad_norm(self, max_norm, out, work):
        """``_grad_norm`` issued into a graph being captured, over the gradients the next step updates.  The chunk
        table must exist from an eager clipped step (raises otherwise).  Returns the table, which the caller keeps
        alive as long as the graph; a replay issues GN_LAUNCHES kernels."""
        return self._grad_norm(list(self._launch_sets(advance=False)), max_norm, out, work, build=False)

    @torch.no_grad()
    def _captured_step(self, hyper, clip=None):
        """Issue the step into a graph being captured: one ``tsr_adam_l2_multi_dev`` launch per (group, step) set, set
        ``i`` reading row ``i`` of ``hyper`` (a device float32 tensor of shape (>= sets, 3)).  With ``clip`` (a device
        float32 tensor whose first element is the coefficient ``_captured_grad_norm`` writes, i.e. ``out[1:]``) the
        launches are ``tsr_adam_l2_multi_dev_clip``.  Chunk tables must exist from an eager step (raises otherwise:
        building one is a host-to-device copy).  Changes no host state; returns the launch list for ``_replay_rows``
        -- it holds the device tables, which the caller keeps alive as long as the graph."""
        sets = list(self._launch_sets(advance=False))
        if len(sets) > hyper.shape[0]:
            raise TactileSRHipError(f"captured Adam step: {len(sets)} launches, hyper buffer has {hyper.shape[0]} rows")
        launches = []
        for i, (group, _, items) in enumerate(sets):
            b1, b2 = group["betas"]
            dev, n_chunks = self._table(items, build=False)
            args = (ptr(dev), _I(n_chunks), ctypes.c_void_p(hyper.data_ptr() + 12 * i), ctypes.c_double(b1),
                    ctypes.c_double(b2), _F(group["eps"]), _F(group["weight_decay"]))
            if clip is None:
                call("tsr_adam_l2_multi_dev", *args, stream())
            else:
                call("tsr_adam_l2_multi_dev_clip", *args, ptr(clip), stream())
            launches.append((group, [st for _, _, st in items], dev))
        return launches

    def _replay_rows(self, launches):
        """Host side of one replay of a captured step: advance ``state["step"]`` of every parameter the graph updates
        and return a fresh pinned (len(launches), 3) float32 tensor of {lr, bc1, bc2_sqrt} rows, formed by
        ``tsr_adam_hyper`` from each group's CURRENT lr -- the floats the eager launch would pass."""
        rows = torch.empty(len(launches), 3, dtype=torch.float32, pin_memory=True)
        base = rows.data_ptr()
        lib = _lib.load()
        for i, (group, states, _) in enumerate(launches):
            for st in states:
                st["step"] += 1
            b1, b2 = group["betas"]
            rc = lib.tsr_adam_hyper(_F(group["lr"]), ctypes.c_double(b1), ctypes.c_double(b2),
                                    _I(int(states[0]["step"].item())), ctypes.c_void_p(base + 12 * i))
            if rc != 0:
                raise TactileSRHipError(f"tsr_adam_hyper failed: status {rc}")
        self.launches += len(launches)
        return rows

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group, step, items in self._launch_sets(advance=True):
            b1, b2 = group["betas"]
            dev, n_chunks = self._table(items)
            call("tsr_adam_l2_multi", ptr(dev), _I(n_chunks), _F(group["lr"]), ctypes.c_double(b1), ctypes.c_double(b2),
                 _F(group["eps"]),
                 _F(group["weight_decay"]), _I(step), stream())
            self.launches += 1
        # the kernel wrote the parameters behind autograd's back: invalidate cached weight packs (TactileSR._plan)
        _lib.bump_param_epoch()
        return loss

    @torch.no_grad()
    def step_clipped(self, max_norm: float) -> torch.Tensor:
        """``torch.nn.utils.clip_grad_norm_(<the parameters of this optimizer with a gradient>, max_norm); step()``
        (cpu/trainer.py:354-361) in GN_LAUNCHES + one launch per (group, step) set, without a host sync.  Returns the
        total norm of the gradients before clipping as a 0-dim device tensor (fresh storage every call); the gradients
        are left clipped, as torch leaves them.  The coefficient is torch's for that norm bit for bit; a NaN gradient
        makes every gradient NaN, an Inf one makes the finite ones 0 (torch's rules)."""
        sets = list(self._launch_sets(advance=True))
        if not sets:                      # nothing to clip or step (torch: a norm of 0)
            _lib.bump_param_epoch()
            return torch.tensor(0.0)
        device = sets[0][2][0][0].device
        out = torch.empty(2, dtype=torch.float32, device=device)           # {total_norm, clip_coef}
        work = torch.empty(GN_PARTIALS, dtype=torch.float64, device=device)
        self._grad_norm(sets, max_norm, out, work)
        self.launches += GN_LAUNCHES
        coef = out[1:]
        for group, step, items in sets:
            b1, b2 = group["betas"]
            dev, n_chunks = self._table(items)
            call("tsr_adam_l2_multi_clip", ptr(dev), _I(n_chunks), _F(group["lr"]), ctypes.c_double(b1),
                 ctypes.c_double(b2), _F(group["eps"]), _F(group["weight_decay"]), _I(step), ptr(coef), stream())
            self.launches += 1
        _lib.bump_param_epoch()
        return out[0]
