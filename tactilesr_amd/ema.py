"""Weight averaging during training: an exponential moving average (EMA) or the equal-weight running mean (SWA) of
every tensor of a model's ``state_dict()``, kept by ONE launch of ``tsr_ema_multi`` per step.

    ema = WeightEMA(model, decay=0.999, warmup=10)          # one STORE launch: the shadow starts as the weights
    train_one_iter(model, optimizer, batch, config, ema=ema)  # ... optimizer.step(); ema.update()
    with ema.applied():                                     # SWAP in, SWAP out: the model runs on the average
        eval_func(model, loader, config)
    save_checkpoint(path, model, optimizer, ema=ema)

* The shadow is one flat device allocation, every tensor padded to 16 bytes; ``ema.shadow`` is a name -> view dict with
  the state dict's keys, shapes and dtypes (``model.load_state_dict(ema.shadow)`` works).  It is fp32 like the weights:
  at ``decay >= 0.9999`` an increment below half an ulp of the average is lost, as in every fp32 EMA.
* Update ``t`` (0-based) is ``avg = fmaf(1 - decay_at(t), src - avg, avg)`` on float parameters and, with
  ``buffers="ema"``, on float buffers (the BatchNorm running statistics); with ``buffers="copy"`` (the default) float
  buffers are copied, and integer buffers (``num_batches_tracked``) always are.  Frozen parameters stay in the table:
  ``src == avg`` leaves the average as it is.
* ``decay_at(t)`` is formed in Python doubles: ``decay``; with ``warmup=w`` ``min(decay, (1 + t) / (w + t))``; with
  ``decay="swa"`` ``t / (t + 1)``, the equal-weight mean of ``torch.optim.swa_utils.AveragedModel``.
* The device chunk table is cached under every address it holds, like ``optim.Adam._table``: tensors that moved (same
  names and shapes) get a new table and keep the shadow; other names or shapes raise ``TactileSRHipError``.
* ``applied()`` exchanges weights and shadow in place, so parameter and buffer addresses -- Adam's chunk tables, a
  captured ``GraphedTrainStep`` -- stay valid; the weight packs and eval plans the model caches are invalidated after
  each swap.  ``update()``, ``applied()``, ``copy_to()``, ``reset()`` and ``load_state_dict()`` raise while applied.
* A captured train step issues ``tsr_ema_multi_dev`` through ``_captured_update`` / ``_replay_scalar``: the launch
  reads ``1 - decay`` from a device float rewritten before every replay, so a warm-up is not frozen by the capture.
* A model on the CPU takes the same class through torch ops with the same formula (the host logic is testable without
  a GPU; the multiply-add is formed in fp64 and rounded, which can differ from the fused one in the last bit).  A model
  whose tensors sit on different devices is refused.

``recalibrate_bn`` recomputes the BatchNorm running statistics for averaged weights (torch's ``update_bn``).
"""
from __future__ import annotations

import contextlib
import ctypes

import torch

from . import _lib
from ._lib import call, stream, c_int as _I, c_float as _F, TactileSRHipError

CHUNK = 4096                               # 4-byte words per record
UPDATE, STORE, LOAD, SWAP = 0, 1, 2, 3     # tsr_ema_multi's op


class _Rec(ctypes.Structure):              # mirror of tsr_ema_chunk (include/tactilesr_hip.h)
    _fields_ = [("avg", ctypes.c_void_p), ("src", ctypes.c_void_p), ("n", ctypes.c_int), ("mode", ctypes.c_int)]


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def _resolve(module):
    """[(name, owner module, attribute, is_parameter)] for every key of ``module.state_dict()``, and the module tree
    as (parent, child name, child) triples: while those hold, ``owner._parameters[attr]`` / ``owner._buffers[attr]`` is
    the live tensor of the key without walking the tree."""
    live = module.state_dict(keep_vars=True)
    items = []
    for name, t in live.items():
        prefix, _, attr = name.rpartition(".")
        try:
            owner = module.get_submodule(prefix)
        except AttributeError:
            owner = None
        is_param = owner is not None and owner._parameters.get(attr) is t
        if not is_param and (owner is None or owner._buffers.get(attr) is not t):
            raise TactileSRHipError(f"WeightEMA: state_dict key {name!r} is not a parameter or buffer of the module "
                                    "tree (a custom state_dict is not supported)")
        items.append((name, owner, attr, is_param))
    tree = [(parent, cname, child) for _, parent in module.named_modules() for cname, child in parent._modules.items()]
    return items, tree


def _spec(t):
    return tuple(t.shape), t.dtype


class WeightEMA:
    def __init__(self, model, decay=0.999, warmup=None, buffers="copy"):
        if buffers not in ("copy", "ema"):
            raise ValueError(f"WeightEMA: buffers is 'copy' or 'ema', got {buffers!r}")
        if decay != "swa" and not (isinstance(decay, (int, float)) and 0.0 <= float(decay) <= 1.0):
            raise ValueError(f"WeightEMA: decay is a number in [0, 1] or 'swa', got {decay!r}")
        if warmup is not None and (decay == "swa" or int(warmup) != warmup or warmup < 1):
            raise ValueError("WeightEMA: warmup is None or an int >= 1 (and has no meaning with decay='swa')")
        self.decay = decay if decay == "swa" else float(decay)
        self.warmup = None if warmup is None else int(warmup)
        self.buffers = buffers
        self.model = model
        self.updates = 0             # updates taken so far: the next one is number `updates`
        self.launches = 0            # launches issued so far, the STORE of the construction included
        self.table_builds = 0
        self._applied = False
        self._tables = {}            # key (every address the table holds) -> (device table, n_chunks)
        self._items, self._tree = _resolve(_unwrap(model))
        live = self._fetch()
        if not live:
            raise TactileSRHipError("WeightEMA: the model has an empty state_dict")
        self.device = self._one_device(live)
        self._specs = [_spec(t) for t in live]
        self._is_param = [it[3] for it in self._items]
        offsets, off = [], 0
        for t in live:
            if (t.numel() * t.element_size()) % 4:
                raise TactileSRHipError(f"WeightEMA: a {t.dtype} tensor of {t.numel()} elements is not a whole number "
                                        "of 4-byte words")
            offsets.append(off)
            off += -(-t.numel() * t.element_size() // 16) * 16
        self._flat = torch.zeros(max(off, 16), dtype=torch.uint8, device=self.device)
        self.shadow = {it[0]: self._flat[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
                       for it, o, t in zip(self._items, offsets, live)}
        self._run(STORE, 0.0, live)

    # ------------------------------------------------------------------ schedule
    def decay_at(self, t: int) -> float:
        """The decay of update number ``t`` (0-based), in Python doubles."""
        if self.decay == "swa":
            return t / (t + 1)
        if self.warmup is None:
            return self.decay
        return min(self.decay, (1 + t) / (self.warmup + t))

    def _omd(self, t: int) -> float:
        return float(1.0 - self.decay_at(t))

    # ------------------------------------------------------------------ the live tensors and their table
    @staticmethod
    def _one_device(tensors):
        devices = {t.device for t in tensors}
        if len(devices) != 1:
            raise TactileSRHipError(f"WeightEMA: the model's tensors sit on different devices ({sorted(map(str, devices))})")
        return devices.pop()

    def _fetch(self):
        return [(o._parameters if is_p else o._buffers)[a] for _, o, a, is_p in self._items]

    def _live(self, model=None):
        """The live tensors in the shadow's order, of this EMA's model or of ``model`` (same names and shapes)."""
        if model is None:
            if any(parent._modules.get(cname) is not child for parent, cname, child in self._tree):
                items, tree = _resolve(_unwrap(self.model))      # a submodule was replaced: look the tensors up again
                if [it[0] for it in items] != [it[0] for it in self._items]:
                    raise TactileSRHipError("WeightEMA: the model's state_dict keys changed since the EMA was made")
                self._items, self._tree = items, tree
            try:
                live = self._fetch()
            except KeyError as e:
                raise TactileSRHipError(f"WeightEMA: the model no longer has the tensor {e}") from None
        else:
            sd = _unwrap(model).state_dict(keep_vars=True)
            if list(sd) != [it[0] for it in self._items]:
                raise TactileSRHipError("WeightEMA: the model's state_dict keys are not the shadow's")
            live = list(sd.values())
        return live

    def _validate(self, live):
        """Shapes, dtypes, layout and device of the live tensors against the shadow.  Run when a table is built (a hit
        of the address key means these tensors were checked before) and on every CPU operation."""
        for it, t, spec in zip(self._items, live, self._specs):
            if t is None or _spec(t) != spec:
                raise TactileSRHipError(f"WeightEMA: {it[0]!r} is {None if t is None else _spec(t)}, the shadow holds {spec}")
            if not t.is_contiguous():
                raise TactileSRHipError(f"WeightEMA: {it[0]!r} is not contiguous")
        if self._one_device(live) != self.device:
            raise TactileSRHipError(f"WeightEMA: the model is on {live[0].device}, the shadow on {self.device}")

    def _modes(self):
        return [0 if dtype == torch.float32 and (is_p or self.buffers == "ema") else 1
                for (_, dtype), is_p in zip(self._specs, self._is_param)]

    def _table(self, live, build=True):
        try:
            key = (self._flat.data_ptr(), self.buffers) + tuple(t.data_ptr() for t in live)
        except AttributeError:             # a tensor was set to None: _validate names it
            key = None
        hit = self._tables.get(key)
        if hit is not None:
            return hit
        self._validate(live)
        if not build:
            raise TactileSRHipError("WeightEMA: no chunk table for these addresses; building one during a graph capture "
                                    "would be a host-to-device copy -- run an eager update first")
        ptrs = [t.data_ptr() for t in live if t.numel()]
        if len(set(ptrs)) != len(ptrs):
            raise TactileSRHipError("WeightEMA: two state_dict keys share one tensor (tied weights are not supported)")
        recs = []
        for t, mode, avg in zip(live, self._modes(), self.shadow.values()):
            words = t.numel() * t.element_size() // 4
            for off in range(0, words, CHUNK):
                recs.append((avg.data_ptr() + 4 * off, t.data_ptr() + 4 * off, min(CHUNK, words - off), mode))
        arr = (_Rec * len(recs))(*recs)
        dev = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).clone().to(self.device)
        if len(self._tables) > 8:
            self._tables.clear()
        self._tables[key] = (dev, len(recs))       # the key is the table (see optim.Adam._table)
        self.table_builds += 1
        return self._tables[key]

    def _run(self, op, omd, live):
        with torch.no_grad():
            if self.device.type == "cpu":
                self._validate(live)
                self._run_cpu(op, omd, live)
            else:
                dev, n_chunks = self._table(live)
                call("tsr_ema_multi", ctypes.c_void_p(dev.data_ptr()), _I(n_chunks), _I(op), _F(omd), stream())
        self.launches += 1

    def _run_cpu(self, op, omd, live):
        """The launch restated with torch ops.  Copies of equal dtype move the bits."""
        omd32 = float(torch.tensor(omd, dtype=torch.float32))
        if not 0.0 <= omd32 <= 1.0:
            raise TactileSRHipError("tsr_ema_multi failed: status 1 (bad argument)")
        for t, mode, avg in zip(live, self._modes(), self.shadow.values()):
            t = t.detach()
            if op == UPDATE and mode == 0:
                diff = t - avg                                      # rounded in fp32
                avg.copy_((omd32 * diff.double() + avg.double()).float())
            elif op in (UPDATE, STORE):
                avg.copy_(t)
            elif op == LOAD:
                t.copy_(avg)
            else:
                tmp = avg.clone()
                avg.copy_(t)
                t.copy_(tmp)

    def _invalidate(self, model=None):
        """The weights or statistics changed behind the model's back: its cached weight packs and eval plans are stale."""
        _lib.bump_param_epoch()
        for m in _unwrap(self.model if model is None else model).modules():
            if hasattr(m, "_plan"):
                m._plan = None

    def _not_applied(self, what):
        if self._applied:
            raise TactileSRHipError(f"WeightEMA.{what} inside applied(): the model holds the average and the shadow the "
                                    "weights")

    # ------------------------------------------------------------------ public
    def update(self) -> None:
        """One averaging launch over every tensor, with the decay of update number ``updates``."""
        self._not_applied("update()")
        self._run(UPDATE, self._omd(self.updates), self._live())
        self.updates += 1

    @contextlib.contextmanager
    def applied(self):
        """Run the body with the averaged weights (and shadow buffers) in the model: SWAP in, SWAP out in a ``finally``."""
        self._not_applied("applied()")
        self._run(SWAP, 0.0, self._live())
        self._applied = True
        self._invalidate()
        try:
            yield self
        finally:
            self._run(SWAP, 0.0, self._live())
            self._applied = False
            self._invalidate()

    def copy_to(self, model=None) -> None:
        """Overwrite the tensors of ``model`` (default: this EMA's model) with the shadow."""
        self._not_applied("copy_to()")
        self._run(LOAD, 0.0, self._live(model))
        self._invalidate(model)

    def reset(self) -> None:
        """Restart the average from the model's current tensors."""
        self._not_applied("reset()")
        self._run(STORE, 0.0, self._live())
        self.updates = 0

    def state_dict(self) -> dict:
        return {"decay": self.decay, "warmup": self.warmup, "buffers": self.buffers, "updates": self.updates,
                "shadow": {k: v.clone() for k, v in self.shadow.items()}}

    def load_state_dict(self, state: dict) -> None:
        self._not_applied("load_state_dict()")
        shadow = state["shadow"]
        if list(shadow) != list(self.shadow):
            odd = sorted(set(shadow) ^ set(self.shadow))
            raise TactileSRHipError(f"WeightEMA.load_state_dict: the keys differ from the shadow's ({odd[:4]}...)")
        for k, v in shadow.items():
            if _spec(v) != _spec(self.shadow[k]):
                raise TactileSRHipError(f"WeightEMA.load_state_dict: {k!r} is {_spec(v)}, the shadow holds "
                                        f"{_spec(self.shadow[k])}")
        if state["buffers"] not in ("copy", "ema"):
            raise TactileSRHipError(f"WeightEMA.load_state_dict: buffers = {state['buffers']!r}")
        with torch.no_grad():
            for k, v in shadow.items():
                self.shadow[k].copy_(v)
        self.decay, self.warmup, self.buffers = state["decay"], state["warmup"], state["buffers"]
        self.updates = int(state["updates"])

    # ------------------------------------------------------------------ the captured step (train/graph.py)
    @torch.no_grad()
    def _captured_update(self, buf):
        """Issue the update into a graph being captured: ``tsr_ema_multi_dev`` reading ``1 - decay`` from ``buf`` (one
        device float32).  The chunk table must exist from an eager update (raises otherwise).  Changes no host state;
        returns the table, which the caller keeps alive as long as the graph."""
        self._not_applied("update()")
        if self.device.type == "cpu" or buf.dtype != torch.float32 or buf.numel() < 1 or buf.device != self.device:
            raise TactileSRHipError("captured EMA update: needs one float32 on the shadow's ROCm device")
        dev, n_chunks = self._table(self._live(), build=False)
        call("tsr_ema_multi_dev", ctypes.c_void_p(dev.data_ptr()), _I(n_chunks), _I(UPDATE),
             ctypes.c_void_p(buf.data_ptr()), stream())
        return dev

    def _replay_scalar(self) -> float:
        """Host side of one replay of a captured update: advance ``updates`` and return the float the eager launch
        would pass for this update."""
        self._not_applied("update()")
        omd = self._omd(self.updates)
        self.updates += 1
        self.launches += 1
        return omd


def recalibrate_bn(model, loader, config) -> int:
    """Recompute the BatchNorm running statistics of ``model`` for its CURRENT weights from the batches of ``loader``
    (torch's ``swa_utils.update_bn``): what SWA or ``WeightEMA(buffers="ema")`` needs before the average is evaluated,
    typically ``with ema.applied(): recalibrate_bn(model, loader, config)``.

    Train-mode FORWARD launches only, under ``no_grad``.  For batch ``k`` (0-based) every BatchNorm layer in
    batch-statistics mode runs with ``momentum = 1 / (k + 1)`` (the train engine reads ``bn.momentum`` per forward), so
    after ``K`` batches ``running_mean`` / ``running_var`` are the equal-weight mean of the ``K`` per-batch statistics and
    ``num_batches_tracked`` has advanced by ``K``.  Each layer's momentum and every module's training flag are restored
    afterwards, also when a forward raises.  Layers in eval mode (``hold_bn_statistics``) are skipped; parameters are
    untouched.  ``loader`` yields ``(LR, HR)`` batches as the trainer's does (HR is not read) or LR tensors.  Returns
    ``K``."""
    module = _unwrap(model)
    device = next(module.parameters()).device
    flags = {m: m.training for m in module.modules()}
    if not module.training:
        module.train()               # TactileSR.train() keeps the layers marked by hold_bn_statistics in eval mode
    layers = [m for m in module.modules()
              if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training and m.track_running_stats]
    momenta = [m.momentum for m in layers]
    k = 0
    try:
        with torch.no_grad():
            for batch in loader:
                LR = batch[0] if isinstance(batch, (tuple, list)) else batch
                LR = LR.to(device).type(torch.float32)[:, :config["seqsCnt"] * config["axisCnt"]]
                for m in layers:
                    m.momentum = 1.0 / (k + 1)
                model(LR)
                k += 1
    finally:
        for m, mom in zip(layers, momenta):
            m.momentum = mom
        for m, flag in flags.items():
            m.training = flag
        _lib.bump_param_epoch()      # eval-mode weight packs fold the running statistics
    return k
