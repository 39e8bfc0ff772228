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

``Adam(amsgrad=True)`` and ``AdamW`` (decoupled weight decay, ``torch.optim.AdamW``; with or without ``amsgrad``)
run the same way through the extended launch ``tsr_adam_multi_ex`` (csrc/adam_ex.hip), whose flags select the
formula; AMSGrad's running maximum is the state tensor ``max_exp_avg_sq`` (torch's key) and reaches the kernel through
a second device table of one pointer per chunk record.  ``Adam`` without ``amsgrad`` stays on ``tsr_adam_l2_multi``.
``decay_param_groups`` splits a model into the no-decay (BatchNorm, biases) and the decay parameter group.

A captured step (``tactilesr_amd.train.graph.GraphedTrainStep``) goes through ``_captured_step`` /
``_replay_rows``: the same kernel body launched through ``tsr_adam_l2_multi_dev`` (``tsr_adam_multi_ex_dev``), which
reads lr and the bias corrections (and AdamW's ``1 - lr * weight_decay``) from a device buffer that is rewritten on
the host before every replay.

Gradient-norm clipping (the reference trainer's ``clip_grad_norm``, cpu/trainer.py:354-356): ``step_clipped(max_norm)``
is ``torch.nn.utils.clip_grad_norm_(<the parameters with a gradient>, max_norm); step()`` without a host sync -- one
``tsr_grad_norm_multi`` (two kernels) over a chunk table of every group's gradients writes {total_norm, clip_coef} to a
device array, then every (group, step) set runs ``tsr_adam_l2_multi_clip`` (the extended launch with ``clip``), which
scales the gradient by that coefficient, writes it back (torch leaves ``p.grad`` clipped) and takes the plain step on it.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import call, ptr, stream, c_int as _I, c_float as _F, TactileSRHipError

CHUNK = 4096
GN_PARTIALS = 256     # tsr_grad_norm_multi: one double partial per workgroup of its first kernel
GN_LAUNCHES = 2       # kernels one tsr_grad_norm_multi call issues
DECOUPLED = 1         # TSR_ADAM_DECOUPLED: p *= 1 - lr * wd instead of g += wd * p
AMSGRAD = 2           # TSR_ADAM_AMSGRAD: divide by the running maximum of exp_avg_sq

_D = ctypes.c_double
_NULL = ctypes.c_void_p(0)


class _Rec(ctypes.Structure):         # mirror of tsr_adam_chunk (include/tactilesr_hip.h)
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_int), ("reserved", ctypes.c_int)]


def _to_device(arr, device):
    return torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).clone().to(device)


class Adam(torch.optim.Optimizer):
    _decoupled = False          # AdamW: the weight decay leaves the gradient and multiplies the parameter

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad)))
        self._tables = {}           # key (every address the table holds) -> (device table, n_chunks[, vmax table])
        self.launches = 0           # kernel launches issued so far (tests: one per step)
        self.table_builds = 0       # device tables built so far (steady state with the gradient arena: exactly one)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:      # an optimizer pickled before the key existed
            group.setdefault("amsgrad", False)

    def _flags(self, group) -> int:
        """The extended launch's flags for a group; 0 is the legacy launch (``tsr_adam_l2_multi`` and its siblings)."""
        return (DECOUPLED if self._decoupled else 0) | (AMSGRAD if group.get("amsgrad", False) else 0)

    @property
    def hyper_width(self) -> int:
        """Floats per row of the device buffer a captured step reads: {lr, bc1, bc2_sqrt} when every group runs the
        legacy launch, {lr, bc1, bc2_sqrt, decay} as soon as one runs the extended launch (a legacy group then reads
        the first three of its row)."""
        return 4 if any(self._flags(g) for g in self.param_groups) else 3

    def load_state_dict(self, state_dict):
        """``torch.optim.Optimizer.load_state_dict``; a state without ``max_exp_avg_sq`` for an AMSGrad group (this
        optimizer's, or the saved group's own ``amsgrad``) raises before anything is loaded."""
        saved = state_dict["param_groups"]
        if len(saved) == len(self.param_groups):      # torch raises on a mismatch itself
            for own, sg in zip(self.param_groups, saved):
                if not (own.get("amsgrad", False) or sg.get("amsgrad", False)):
                    continue
                for pid in sg["params"]:
                    st = state_dict["state"].get(pid)
                    if st and "max_exp_avg_sq" not in st:
                        raise KeyError("tactilesr_amd.optim: this state has no 'max_exp_avg_sq' for a parameter of an "
                                       "amsgrad=True group (it was saved without AMSGrad)")
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)

    def _table(self, items, build=True, vmax=False):
        """The device chunk table of ``items`` as (table, n_chunks), built once per set of addresses.  ``vmax=True``
        adds the table of ``max_exp_avg_sq`` pointers, one per record: (table, n_chunks, vmax table), cached under a
        key that holds those addresses too."""
        key = tuple((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                    + ((st["max_exp_avg_sq"].data_ptr(),) if vmax else ()) for p, g, st in items)
        hit = self._tables.get(key)
        if hit is not None:
            return hit
        if not build:
            raise TactileSRHipError("tactilesr_amd.optim.Adam: no chunk table for these (param, grad, state) addresses; "
                                    "building one during a graph capture would be a host-to-device copy -- run an eager "
                                    "step with the same gradients first")
        recs, vptr = [], []
        for p, g, st in items:
            n = p.numel()
            for off in range(0, n, CHUNK):
                b = 4 * off
                recs.append((p.data_ptr() + b, g.data_ptr() + b, st["exp_avg"].data_ptr() + b,
                             st["exp_avg_sq"].data_ptr() + b, min(CHUNK, n - off), 0))
                if vmax:
                    vptr.append(st["max_exp_avg_sq"].data_ptr() + b)
        arr = (_Rec * len(recs))(*recs)
        device = items[0][0].device
        dev = _to_device(arr, device)
        if len(self._tables) > 8:
            self._tables.clear()
        # The key IS the table: every address a record holds (param, grad, exp_avg, exp_avg_sq of every tensor) is part
        # of it, so a hit is valid whatever lived at those addresses in between -- no tensor has to be kept alive for
        # it (holding the gradients here pinned up to nine stale gradient sets of a model whose gradients are fresh
        # autograd tensors every step).
        if vmax:
            self._tables[key] = (dev, len(recs), _to_device((ctypes.c_void_p * len(vptr))(*vptr), device))
        else:
            self._tables[key] = (dev, len(recs))
        self.table_builds += 1
        return self._tables[key]

    def _launch_sets(self, advance):
        """Yields (group, step, [(p, grad, state)]) in launch order: per group, the parameters with a gradient, split by
        their (1-based) step number.  ``advance`` increments ``state["step"]`` (the eager step, group by group as it
        launches); without it the step number is the one the next step will use and nothing is created or changed."""
        for group in self.param_groups:
            ams = bool(group.get("amsgrad", False))
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
                        if ams:
                            st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["step"] += 1
                    step = int(st["step"].item())      # CPU scalar: no device sync
                else:
                    if len(st) == 0 or not g.is_contiguous():
                        raise TactileSRHipError("tactilesr_amd.optim.Adam: a captured step needs the optimizer state "
                                                "and contiguous gradients of an eager step first")
                    step = int(st["step"].item()) + 1
                if ams and "max_exp_avg_sq" not in st:
                    raise TactileSRHipError("tactilesr_amd.optim.Adam: amsgrad=True, but the state of a parameter has no "
                                            "'max_exp_avg_sq' (it was created or loaded without AMSGrad)")
                by_step.setdefault(step, []).append((p, g, st))
            for step, items in by_step.items():
                yield group, step, items

    def _grad_norm(self, sets, max_norm, out, work, build=True):
        """Issue ``tsr_grad_norm_multi`` over the gradients of every (param, grad) item of ``sets`` (as
        ``_launch_sets`` yields them): out = {total_norm, clip_coef} (a device float32 tensor of >= 2 elements), work
        a device float64 tensor of >= GN_PARTIALS elements.  Returns the chunk table the launch reads."""
        if out.dtype != torch.float32 or out.numel() < 2 or work.dtype != torch.float64 or work.numel() < GN_PARTIALS:
            raise TactileSRHipError("gradient norm: out needs 2 float32 elements, work GN_PARTIALS float64 elements")
        # with AMSGrad everywhere the step's own table (one group: the very same records) serves the norm too
        vmax = all(group.get("amsgrad", False) for group, _, _ in sets)
        dev, n_chunks = self._table([it for _, _, items in sets for it in items], build=build, vmax=vmax)[:2]
        call("tsr_grad_norm_multi", ptr(dev), _I(n_chunks), _F(max_norm), ptr(work), ptr(out), stream())
        return dev

    @torch.no_grad()
    def _captured_grad_norm(self, max_norm, out, work):
        """``_grad_norm`` issued into a graph being captured, over the gradients the next step updates.  The chunk
        table must exist from an eager clipped step (raises otherwise).  Returns the table, which the caller keeps
        alive as long as the graph; a replay issues GN_LAUNCHES kernels."""
        return self._grad_norm(list(self._launch_sets(advance=False)), max_norm, out, work, build=False)

    def _launch(self, group, items, step=None, hyper=None, clip=None, build=True):
        """One step launch over ``items`` of ``group``: the host-scalar form with ``step``, the device-scalar form with
        ``hyper`` (the address of the set's row); ``clip`` is the device coefficient or None.  The legacy entry points
        when the group's flags are 0, the extended launch otherwise.  Returns the device tables it reads."""
        flags = self._flags(group)
        b1, b2 = group["betas"]
        tail = (_D(b1), _D(b2), _F(group["eps"]), _F(group["weight_decay"]))
        if not flags:
            dev, n_chunks = self._table(items, build=build)
            name = "tsr_adam_l2_multi" + ("" if hyper is None else "_dev") + ("" if clip is None else "_clip")
            head = (ptr(dev), _I(n_chunks)) + ((_F(group["lr"]),) if hyper is None else (hyper,))
            call(name, *head, *tail, *(() if hyper is not None else (_I(step),)), *(() if clip is None else (ptr(clip),)),
                 stream())
            return (dev,)
        if flags & AMSGRAD:
            dev, n_chunks, vdev = self._table(items, build=build, vmax=True)
        else:
            dev, n_chunks = self._table(items, build=build)
            vdev = None
        head = (ptr(dev), ptr(vdev), _I(n_chunks), _I(flags))
        cp = _NULL if clip is None else ptr(clip)
        if hyper is None:
            call("tsr_adam_multi_ex", *head, _F(group["lr"]), *tail, _I(step), cp, stream())
        else:
            call("tsr_adam_multi_ex_dev", *head, hyper, *tail, cp, stream())
        return (dev, vdev)

    @torch.no_grad()
    def _captured_step(self, hyper, clip=None):
        """Issue the step into a graph being captured: one ``tsr_adam_l2_multi_dev`` (``tsr_adam_multi_ex_dev``) launch
        per (group, step) set, set ``i`` reading row ``i`` of ``hyper`` (a device float32 tensor of shape
        (>= sets, ``hyper_width``)).  With ``clip`` (a device float32 tensor whose first element is the coefficient
        ``_captured_grad_norm`` writes, i.e. ``out[1:]``) the launches are the clipping forms.  Chunk tables must exist
        from an eager step (raises otherwise: building one is a host-to-device copy).  Changes no host state; returns
        the launch list for ``_replay_rows`` -- it holds the device tables, which the caller keeps alive as long as the
        graph."""
        sets = list(self._launch_sets(advance=False))
        if len(sets) > hyper.shape[0]:
            raise TactileSRHipError(f"captured Adam step: {len(sets)} launches, hyper buffer has {hyper.shape[0]} rows")
        width = self.hyper_width
        if hyper.dim() != 2 or hyper.shape[1] != width or not hyper.is_contiguous() or hyper.dtype != torch.float32:
            raise TactileSRHipError(f"captured Adam step: the hyper buffer needs contiguous float32 rows of {width} "
                                    f"(optimizer.hyper_width), got {tuple(hyper.shape)}")
        launches = []
        for i, (group, _, items) in enumerate(sets):
            row = ctypes.c_void_p(hyper.data_ptr() + 4 * width * i)
            dev = self._launch(group, items, hyper=row, clip=clip, build=False)
            launches.append((group, [st for _, _, st in items], dev))
        return launches

    def _replay_rows(self, launches):
        """Host side of one replay of a captured step: advance ``state["step"]`` of every parameter the graph updates
        and return a fresh pinned (len(launches), ``hyper_width``) float32 tensor of {lr, bc1, bc2_sqrt} rows
        ({lr, bc1, bc2_sqrt, decay} with the extended launch), formed by ``tsr_adam_hyper`` (``tsr_adam_hyper_ex``)
        from each group's CURRENT lr -- the floats the eager launch would pass."""
        width = self.hyper_width
        rows = torch.empty(len(launches), width, dtype=torch.float32, pin_memory=True)
        if width == 4:
            rows[:, 3] = 1.0        # a legacy group's launch does not read it
        base = rows.data_ptr()
        lib = _lib.load()
        for i, (group, states, _) in enumerate(launches):
            for st in states:
                st["step"] += 1
            b1, b2 = group["betas"]
            flags = self._flags(group)
            step, row = _I(int(states[0]["step"].item())), ctypes.c_void_p(base + 4 * width * i)
            if not flags:
                name, rc = "tsr_adam_hyper", lib.tsr_adam_hyper(_F(group["lr"]), _D(b1), _D(b2), step, row)
            else:
                name, rc = "tsr_adam_hyper_ex", lib.tsr_adam_hyper_ex(_F(group["lr"]), _D(b1), _D(b2), step,
                                                                      _F(group["weight_decay"]), _I(flags), row)
            if rc != 0:
                raise TactileSRHipError(f"{name} failed: status {rc}")
        self.launches += len(launches)
        return rows

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group, step, items in self._launch_sets(advance=True):
            self._launch(group, items, step=step)
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
            self._launch(group, items, step=step, clip=coef)
            self.launches += 1
        _lib.bump_param_epoch()
        return out[0]


class AdamW(Adam):
    """``torch.optim.AdamW``: Adam with DECOUPLED weight decay -- ``p *= 1 - lr * weight_decay``, then the Adam step on
    the bare gradient -- in one ``tsr_adam_multi_ex`` launch per (group, step) set.  Everything ``Adam`` does (clipping
    fused into the step, the captured step, torch's state keys) holds; ``amsgrad=True`` adds ``max_exp_avg_sq``."""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)


def decay_param_groups(model, weight_decay, lr=None):
    """Two param groups for ``Adam`` / ``AdamW``: first the parameters of ``nn.BatchNorm2d`` layers and every parameter
    with ``dim() <= 1`` (biases) at ``weight_decay=0``, then the rest at ``weight_decay``; ``lr`` (optional) is set on
    both.  Inside a group the order is ``model.parameters()``'s; frozen parameters are kept (the step skips a parameter
    without a gradient).  Two groups are two launches per step."""
    bn = {id(p) for mod in model.modules() if isinstance(mod, torch.nn.BatchNorm2d) for p in mod.parameters(recurse=False)}
    no_decay, decay = [], []
    for p in model.parameters():
        (no_decay if id(p) in bn or p.dim() <= 1 else decay).append(p)
    groups = [dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=float(weight_decay))]
    if lr is not None:
        for g in groups:
            g["lr"] = lr
    return groups
