"""HIP-graph replay of the training step for small batches.

At the reference's train batch (``train_batch_size = 32``, config/default.py:46) the HIP train step is ~490 launches
of a few microseconds each: the HOST's launch path, not the GPU, sets its time.  ``GraphedTrainStep`` captures one
whole step -- ``train_one_iter``'s zero_grad, ``train_cal_loss``, backward and Adam (train/tactileSR_train.py:41-51,
cpu/trainer.py:346-362) -- into one HIP graph (``torch.cuda.CUDAGraph``, one stream) and replays it with one host call.
Opt-in; the plain ``train_one_iter`` path is untouched.

    gstep = GraphedTrainStep(model, optimizer, config, warmup=1)    # model.train() on the ROCm device, optim.Adam
    loss_dict = gstep((LR, HR_raw))                                 # every call is ONE training step

* The first ``warmup`` calls run ``train_one_iter`` eagerly (real steps): the first backward lays out the gradient
  arena (tactilesr_amd.ddp), the first Adam step builds its chunk table and the state, one-time kernel attributes are
  set.  The next call captures a step and replays it once; later calls copy the batch into the static inputs and
  replay.
* lr and Adam's bias corrections are NOT frozen by the capture: the graph's Adam launch (``tsr_adam_l2_multi_dev``)
  reads them from a device buffer that is rewritten before every replay from the optimizer's CURRENT ``group["lr"]``
  (an lr scheduler works unchanged) and the advanced ``state["step"]``.  The step then has the eager step's results
  bit for bit, checkpoints included.
* Recapture: when ``train_impl``, the parameter / buffer / optimizer-state / gradient-arena addresses, the set of
  parameters that require grad (the captured backward holds only the launches a trainable parameter depends on), the set
  of BatchNorm layers in eval mode (``hold_bn_statistics``: their statistics launches are not in the capture), the loss
  config (one ``SRLossSpec``, parsed from the optional ``ssim_*``, ``pixel_loss*`` / ``contact_*``, ``degradation_*`` and
  ``sample_weight_norm`` keys: the captured loss and the returned dict are ``sr_step_loss``'s, the function
  ``train_cal_loss`` itself calls -- here outside autograd, on the static buffers, the z-taxels a channel slice of the
  static ``LR`` -- so the launches are those of ``functional.sr_loss_fwd_bwd`` in both steps),
  the optimizer's baked constants (``betas``, ``eps``, ``weight_decay``) or ``clip_grad_norm`` change, the graph is dropped and the next ``warmup`` calls run eagerly again before a new capture.  ``captures`` counts the captures.
* The returned ``total_loss`` is the graph's static OUTPUT BUFFER (like ``GraphedForward``): the next call overwrites
  it, so clone it to keep it.  It carries no autograd graph.
* The captured step is one stream of launches: the train engine's forward and backward and the loss are driven
  directly, not through the autograd engine (whose per-node streams would fork the capture), so autograd hooks on the
  parameters do not run in it.
* Memory: the activations of one step live in the graph's private memory pool, ON TOP of what the eager warm-up left
  in the caching allocator.  Large batches work but are not the target.
* Gradient-norm clipping: ``GraphedTrainStep(..., clip_grad_norm=c)`` with ``c > 0`` is ``train_one_iter(...,
  clip_grad_norm=c)`` (the reference ``Trainer(clip_grad_norm=c)``, cpu/trainer.py:354-356).  The eager warm-up calls
  pass ``c`` on; the capture issues the norm kernels (``tsr_grad_norm_multi``, into a static work buffer and a static
  {total_norm, clip_coef} array allocated before the capture) and the Adam launches in their clipping form
  (``tsr_adam_l2_multi_dev_clip``, reading the coefficient from that array), so every replay clips with the norm of
  its own gradients.  ``c`` is baked into the graph like ``betas`` / ``eps`` / ``weight_decay``: assigning another
  ``gstep.clip_grad_norm`` drops the graph and recaptures.  Clipping needs the fused path's condition: every trainable
  model parameter is stepped by the optimizer (refused otherwise, e.g. the Seqs transplant, whose new parameters are
  not in the optimizer; ``model_param_init(..., freeze=True)`` freezes them and the flow is accepted).  ``c <= 0`` (the
  default) captures the step as before.
* Weight averaging: ``GraphedTrainStep(..., ema=e)`` with a ``tactilesr_amd.WeightEMA`` is ``train_one_iter(..., ema=e)``.
  The eager warm-up calls pass ``e`` on (the first ``e.update()`` builds its chunk table); the capture issues the
  averaging launch after the Adam launches in its device-scalar form (``tsr_ema_multi_dev``), and ``1 - decay`` of each
  replay -- ``e.decay_at(e.updates)``, so a warm-up or ``"swa"`` schedule is not frozen by the capture -- is written into
  a static one-float device buffer before that replay.  The shadow is then the eager step's bit for bit.  The identity of
  ``e``, its shadow address and its ``buffers`` mode are baked in: another or a re-allocated EMA recaptures.  ``ema=None``
  (the default) captures the step as before.
* Per-sample gamma: a batch may be ``(LR, HR_raw, gamma)`` with ``gamma`` (B,) fp32; it is copied into a third static
  buffer that the captured degradation launch reads, and its shape joins the batch signature.
* Per-sample supervision weights: a batch may be ``(LR, HR_raw, gamma, weight)`` (``gamma`` may be ``None``) with
  ``weight`` (B,) fp32; it is copied into a fourth static buffer that the captured scale launch
  (``functional.sample_scale``) reads, so the weights are data: replays with different weights -- all-zero included --
  need no recapture.  Its shape and dtype join the batch signature and ``sample_weight_norm`` the key (a changed norm
  recaptures).  The returned dict is ``train_cal_loss``'s for such a batch (``labeled_weight`` included).
* Refused (``TactileSRHipError``): eval mode, a batch whose shape / dtype differs from the first call's, an attached
  ``GradSync`` (no collectives inside a graph), ``engine.profile`` / ``engine.debug`` / ``engine.keep_ctx``, an
  optimizer other than ``tactilesr_amd.optim.Adam``, a model not on a ROCm device, a model without a trainable
  parameter, clipping where a trainable model parameter is not in the optimizer, a call inside ``ema.applied()``.
"""
from __future__ import annotations

import torch

from .. import _lib
from .. import optim as opt_mod
from .._lib import TactileSRHipError
from ..ddp import note_forward
from .tactileSR_train import SRLossSpec, _batch_gamma, _batch_weight, _degradation_gamma, _prep, sr_step_loss, train_one_iter

_CONFIG_KEYS = ("HR_scale_num", "scale_factor", "seqsCnt", "axisCnt")      # what the captured train_cal_loss bakes in


class GraphedTrainStep:
    def __init__(self, model, optimizer, config, warmup: int = 1, clip_grad_norm: float = 0.0, ema=None):
        from .. import optim
        p0 = next(model.parameters(), None)
        if p0 is None or not p0.is_cuda:
            raise TactileSRHipError("GraphedTrainStep needs the model on a ROCm device (no CPU fallback)")
        if not hasattr(model, "train_engine"):
            raise TactileSRHipError(f"GraphedTrainStep trains a tactilesr_amd.TactileSR, got {type(model).__name__}")
        if not isinstance(optimizer, optim.Adam):
            raise TactileSRHipError("GraphedTrainStep needs tactilesr_amd.optim.Adam (its step reads lr and the bias "
                                    f"corrections from device memory on replay), got {type(optimizer).__name__}")
        if int(warmup) < 1:
            raise TactileSRHipError("GraphedTrainStep needs warmup >= 1 (the first backward lays out the gradient arena)")
        if ema is not None and getattr(ema.model, "module", ema.model) is not getattr(model, "module", model):
            raise TactileSRHipError("GraphedTrainStep: ema averages another model")
        self.model, self.optimizer, self.config = model, optimizer, config
        self.warmup = int(warmup)
        self.clip_grad_norm = float(clip_grad_norm)
        self.ema = ema
        self.captures = 0
        self._sig = None             # (shape, dtype) of LR and HR_raw, fixed by the first call
        self._drop()

    def _drop(self) -> None:
        self.graph = None
        self._out = self._launches = self._hyper = self._LR = self._HR = self._G = self._SW = None
        self._norm = self._norm_work = self._norm_table = None
        self._ema_omd = self._ema_table = None
        self._graph_key = None
        self._eager_left = self.warmup

    def _key(self):
        """Everything the captured step bakes in (addresses and constants); lr and the step number are not."""
        m, opt = self.model, self.optimizer
        arena = m.train_engine().arena
        groups = tuple((tuple(g["betas"]), g["eps"], g["weight_decay"], opt._flags(g),
                        tuple((p.data_ptr(),) + tuple(opt.state[p][k].data_ptr()
                                                      for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if k in opt.state[p])
                              for p in g["params"]))
                       for g in opt.param_groups)
        return (m.train_impl, id(arena), arena.flat.data_ptr() if arena is not None else 0,
                tuple(t.data_ptr() for t in m.parameters()), tuple(b.data_ptr() for b in m.buffers()), groups,
                tuple(self.config[k] for k in _CONFIG_KEYS), SRLossSpec.from_config(self.config), self.clip_grad_norm,
                (id(self.ema), self.ema._flat.data_ptr(), self.ema.buffers) if self.ema is not None else None,
                tuple(p.requires_grad for p in m.parameters()),      # the captured backward holds the trainable set's launches
                tuple(mod.training for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)))      # and each BatchNorm's mode

    def _check(self, LR, HR, gamma=None, weight=None) -> None:
        m = self.model
        if not m.training:
            raise TactileSRHipError("GraphedTrainStep replays the TRAIN step: the model is in eval mode")
        if not any(p.requires_grad for p in m.parameters()):
            raise TactileSRHipError("GraphedTrainStep: no model parameter requires grad (nothing to train)")
        sig = (tuple(LR.shape), LR.dtype, tuple(HR.shape), HR.dtype)
        if gamma is not None:                    # a 3-tuple batch: the per-sample gamma is a third static input
            sig += (tuple(gamma.shape), gamma.dtype)
        if weight is not None:                   # a 4-tuple batch: the supervision weights are a fourth static input
            sig += ("weight", tuple(weight.shape), weight.dtype)
        if self._sig is None:
            self._sig = sig
        elif sig != self._sig:
            raise TactileSRHipError(f"GraphedTrainStep was set up for batch (LR, HR_raw[, gamma[, weight]]) of shape / dtype {self._sig}, "
                                    f"got {sig}")
        eng = m.train_engine()
        if eng.grad_sync is not None:
            raise TactileSRHipError("GraphedTrainStep: a GradSync is attached (no collectives inside a graph)")
        if eng.profile is not None or eng.debug is not None or eng.keep_ctx:
            raise TactileSRHipError("GraphedTrainStep: engine.profile / engine.debug / engine.keep_ctx is on "
                                    "(host-side hooks cannot run inside a replayed graph)")
        if self.ema is not None:
            self.ema._not_applied("update()")      # before the replay advances any host state
        if self.clip_grad_norm > 0:
            stepped = {id(p) for g in self.optimizer.param_groups for p in g["params"]}
            if any(p.requires_grad and id(p) not in stepped for p in m.parameters()):
                raise TactileSRHipError("GraphedTrainStep: clip_grad_norm needs every trainable model parameter in the "
                                        "optimizer (the norm is taken over model.parameters(), the fused clip over "
                                        "the optimizer's)")

    def _capture(self, LR, HR, gamma=None, weight=None) -> None:
        m, opt = self.model, self.optimizer
        dev = next(m.parameters()).device
        spec = SRLossSpec.from_config(self.config)      # refuses a bad key before anything is captured
        if gamma is not None:
            self._G = torch.empty(gamma.shape, dtype=torch.float32, device=dev)
        deg_gamma = _degradation_gamma(spec, self._G)
        if weight is not None:
            self._SW = torch.empty(weight.shape, dtype=torch.float32, device=dev)
        self._LR = torch.empty(LR.shape, dtype=LR.dtype, device=dev)
        self._HR = torch.empty(HR.shape, dtype=HR.dtype, device=dev)
        # one row of {lr, bc1, bc2_sqrt} ({lr, bc1, bc2_sqrt, decay}: AdamW, AMSGrad) per Adam launch; at most one
        # launch per parameter
        self._hyper = torch.zeros(max(1, sum(len(g["params"]) for g in opt.param_groups)), opt.hyper_width,
                                  dtype=torch.float32, device=dev)
        clip = self.clip_grad_norm > 0
        if clip:                                 # {total_norm, clip_coef} and the partials of the norm kernels
            self._norm = torch.zeros(2, dtype=torch.float32, device=dev)
            self._norm_work = torch.zeros(opt_mod.GN_PARTIALS, dtype=torch.float64, device=dev)
        if self.ema is not None:                 # 1 - decay of the replay, rewritten before each one
            self._ema_omd = torch.zeros(1, dtype=torch.float32, device=dev)
        eng = m.train_engine()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            # train_one_iter's launches, with the train engine and the loss driven directly instead of through the
            # autograd engine: autograd would run the parameters' AccumulateGrad nodes on the stream each node was
            # created on (the default stream for nodes a live eager graph still holds), i.e. fork the capture.  What
            # autograd adds on top of these launches is dout = dy * 1 (exact) and the .grad assignment done below;
            # grad mode is off as inside the autograd Function's forward and backward.
            LR, HR = _prep((self._LR, self._HR), self.config, dev)
            if LR.shape[1] != m.seqsCnt * m.axisCnt:
                raise TactileSRHipError("input channel should be same with seqsCnt x axisCnt!")
            out, ctx = eng.forward(LR.detach().float().contiguous())
            m._plan = None                       # as TactileSR.forward: running statistics change in place
            named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
            if named:
                note_forward(eng, ctx)
            # train_cal_loss's loss and loss_dict, on the static buffers (the z-taxels are a slice of the static LR)
            _, dy, out_dict = sr_step_loss(spec, out, LR, HR, deg_gamma, self._SW, autograd=False)
            opt.zero_grad()
            grads = eng.backward(ctx, dy)
            del ctx
            missing = [n for n, _ in named if n not in grads]
            if missing:
                raise TactileSRHipError(f"backward produced no gradient for {missing[:4]}...")
            for n, p in named:
                p.grad = grads[n]                # gradient-arena views, as autograd leaves them
            if clip:     # _check holds: zero_grad cleared every other gradient, so fused_clip_applies(m, opt) too
                norm_table = opt._captured_grad_norm(self.clip_grad_norm, self._norm, self._norm_work)
            launches = opt._captured_step(self._hyper, clip=self._norm[1:] if clip else None)
            if self.ema is not None:
                ema_table = self.ema._captured_update(self._ema_omd)
        # the launches (and the norm launch) hold the Adam chunk tables the graph reads: keep them alive with it
        self.graph, self._out, self._launches = graph, out_dict, launches
        self._norm_table = norm_table if clip else None
        self._ema_table = ema_table if self.ema is not None else None      # kept alive with the graph
        self._graph_key = self._key()
        self.captures += 1

    def __call__(self, batch):
        LR, HR = batch[0], batch[1]
        gamma = _batch_gamma(batch, LR.device)
        weight = _batch_weight(batch, LR.device)
        self._check(LR, HR, gamma, weight)
        if self.graph is not None and self._key() != self._graph_key:
            self._drop()
        if self.graph is None and self._eager_left > 0:
            self._eager_left -= 1
            return train_one_iter(self.model, self.optimizer, batch, self.config, clip_grad_norm=self.clip_grad_norm,
                                  ema=self.ema)
        if self.graph is None:
            self._capture(LR, HR, gamma, weight)
        self._LR.copy_(LR)
        self._HR.copy_(HR)
        if gamma is not None:
            self._G.copy_(gamma)
        if weight is not None:
            self._SW.copy_(weight)
        rows = self.optimizer._replay_rows(self._launches)       # advances state["step"]; a fresh pinned tensor
        if self._norm_table is not None:
            self.optimizer.launches += opt_mod.GN_LAUNCHES
        self._hyper[:rows.shape[0]].copy_(rows, non_blocking=True)
        if self.ema is not None:
            self._ema_omd.copy_(torch.tensor([self.ema._replay_scalar()], dtype=torch.float32).pin_memory(),
                                non_blocking=True)
        self.graph.replay()
        # the graph's Adam wrote the parameters and its forward the running statistics: cached weight packs are stale
        _lib.bump_param_epoch()
        return self._out
