"""Host-side mirror of the reference's SR trainer glue (train/tactileSR_train.py:29-101) on the
HIP path.  The reference subclasses its vendored ``cpu.Trainer`` (out of scope here); what the hot
path needs from it are the three functions below with the same argument meaning:

  * ``train_cal_loss(model, batch, config)``  <->  Trainer_tactileSR.train_cal_loss   (:41-51)
  * ``train_one_iter(model, optimizer, batch, config)``  <->  Trainer.train_one_iter  (cpu/trainer.py:346-362),
    its ``clip_grad_norm`` option included
  * ``eval_func(model, test_loader, config)``  <->  eval_func (:66-101), returning the three averages
    the reference only logs.
"""
from __future__ import annotations

import dataclasses
import math
import typing

import torch

from .. import functional as Fh
from .._lib import TactileSRHipError


def default_config():
    """The keys of the reference's tactileSR_config that the path reads (config/default.py:45-72)."""
    return dict(HR_scale_num=10, sensorMaxVaule_factor=250, scale_factor=10, seqsCnt=1, axisCnt=3,
                lr=1e-3, weight_decay=1e-2, train_batch_size=32, test_batch_size=8)


def _prep(batch, config, device):
    LR, HR = batch[0], batch[1]          # a third element (the per-sample gamma) is read by _batch_gamma
    LR, HR = LR.to(device), HR.to(device)
    HR = Fh.prepare_target(HR, config["HR_scale_num"], config["scale_factor"])
    LR = LR.type(torch.float32)[:, :config["seqsCnt"] * config["axisCnt"]]
    return LR, HR


def _batch_gamma(batch, device):
    """The (B,) fp32 per-sample gamma of a batch ``(LR, HR, gamma)`` or ``(LR, HR, gamma, weight)`` on ``device``;
    ``None`` for a 2-tuple and for a 4-tuple whose ``gamma`` is ``None``."""
    if len(batch) == 2:
        return None
    if len(batch) not in (3, 4):
        raise TactileSRHipError("a batch is (LR, HR), (LR, HR, gamma) or (LR, HR, gamma, weight) with gamma a (B,) "
                                f"tensor or None, got {len(batch)} elements")
    g = batch[2]
    if g is None and len(batch) == 4:
        return None
    if not isinstance(g, torch.Tensor) or g.dim() != 1 or g.shape[0] != batch[0].shape[0]:
        raise TactileSRHipError("the third element of a batch is the per-sample gamma, a (B,) tensor")
    return g.to(device).float()


def _batch_weight(batch, device):
    """The (B,) fp32 supervision weights of a 4-tuple batch ``(LR, HR, gamma, weight)`` on ``device``, else ``None``."""
    if len(batch) != 4:
        return None
    w = batch[3]
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] != batch[0].shape[0]:
        raise TactileSRHipError("the fourth element of a batch is the per-sample supervision weight, a (B,) tensor")
    return w.to(device).float()


def sample_weight_config(config):
    """The optional key ``sample_weight_norm`` (default ``"sum"``), read when a batch carries per-sample weights:
    ``"sum"`` makes the supervised terms means over the labeled weight, ``"batch"`` keeps the divisor ``B``
    (``functional.sample_scale``).  An unknown value raises ``TactileSRHipError`` here, before any launch."""
    return Fh.sample_weight_norm_arg(config.get("sample_weight_norm", "sum"))


def ssim_loss_config(config):
    """The optional loss keys ``(ssim_loss_weight, ssim_window, ssim_sigma, ssim_data_range)``, defaults
    ``(0.0, 11, 1.5, 1.0)``.  A weight of 0 (or no key) is the reference's loss, nn.MSELoss alone
    (train/tactileSR_train.py:49); otherwise the loss is ``MSE + weight * (1 - mean_b ssim_b)`` with the windowed
    (``ssim_window`` odd in 3..11) or global (``ssim_window = 0``) SSIM of ``functional.ssim``."""
    return (float(config.get("ssim_loss_weight", 0.0)), int(config.get("ssim_window", 11)),
            float(config.get("ssim_sigma", 1.5)), float(config.get("ssim_data_range", 1.0)))


def pixel_loss_config(config):
    """The optional pixel-criterion keys ``(pixel_loss, pixel_loss_param, contact_loss_weight, contact_threshold)``,
    defaults ``("mse", None, 0.0, 0.0)``: the criterion is ``mean_p w_p rho(out_p - HR_p)`` with ``rho`` the ``"mse"``
    (the reference's nn.MSELoss, train/tactileSR_train.py:49), ``"l1"``, ``"charbonnier"`` (``pixel_loss_param`` = eps,
    default 1e-3) or ``"huber"`` (delta, default 1.0) of ``functional.pixel_loss`` and
    ``w_p = 1 + contact_loss_weight * [HR_p > contact_threshold]`` on the prepared target (after ``/HR_scale_num`` and
    the resize).  Returned as the launch takes them, ``(name, param, weight, threshold)`` with the default parameter
    filled in; an unknown name or a value the kernel would refuse raises ``TactileSRHipError`` here, before any launch."""
    return Fh.pixel_loss_args(config.get("pixel_loss", "mse"), config.get("pixel_loss_param", None),
                              config.get("contact_loss_weight", 0.0), config.get("contact_threshold", 0.0))


def degradation_loss_config(config):
    """The optional degradation-consistency keys, returned as ``(weight, gamma, channel, gain)``:

    * ``degradation_loss_weight`` (default 0: off) -- the weight of ``mean_b q_b``, ``q_b`` the mean squared difference
      between the SR output pooled onto the taxels by the sensor model (``functional.degrade``) and the z-taxels the
      output was computed from;
    * ``degradation_gamma`` -- the mask width, a float in (0, 1e6], for every sample; ``None`` when absent: a non-zero weight
      then needs a batch that carries its own ``gamma`` (a 3-tuple), which also overrides this key;
    * ``degradation_channel`` (default ``axisCnt - 1``, the z axis of the first frame) -- the channel of the prepared
      ``LR`` that holds the z-taxels;
    * ``degradation_gain`` (default ``HR_scale_num``) -- undoes the ``/HR_scale_num`` of the prepared target.

    With weight 0 the other keys are not read.  A bad value raises ``TactileSRHipError`` here, before any launch."""
    try:
        w = float(config.get("degradation_loss_weight", 0.0))
    except (TypeError, ValueError) as e:
        raise TactileSRHipError(f"degradation_loss_weight: {e}") from None
    if not math.isfinite(w):
        raise TactileSRHipError(f"degradation_loss_weight must be finite, got {w}")
    if w == 0:
        return 0.0, None, None, None
    gamma = config.get("degradation_gamma", None)
    if gamma is not None:
        if isinstance(gamma, torch.Tensor):
            raise TactileSRHipError("degradation_gamma is a float; a per-sample gamma travels with the batch")
        gamma = Fh.degrade_gamma_arg(gamma, 0)[1]
    n_ch = int(config["seqsCnt"]) * int(config["axisCnt"])
    ch = config.get("degradation_channel", int(config["axisCnt"]) - 1)
    if isinstance(ch, bool) or not isinstance(ch, int) or not 0 <= ch < n_ch:
        raise TactileSRHipError(f"degradation_channel must be an int in [0, {n_ch}), got {ch!r}")
    try:
        gain = float(config.get("degradation_gain", config["HR_scale_num"]))
    except (TypeError, ValueError) as e:
        raise TactileSRHipError(f"degradation_gain: {e}") from None
    if not math.isfinite(gain):
        raise TactileSRHipError(f"degradation_gain must be finite, got {gain}")
    return w, gamma, ch, gain


def contact_readout_config(config):
    """The optional contact-readout keys, returned as ``(threshold, mode, gain, span)`` the way
    ``functional.contact_metrics`` takes them:

    * ``contact_threshold`` (default 0.0) -- the key the contact weight of ``pixel_loss_config`` already reads: the
      contact is ``HR > contact_threshold`` on the prepared target, and the same rule is applied to the output;
    * ``contact_threshold_mode`` (default ``"abs"``) -- ``"range"`` makes the threshold a fraction in [0, 1) of each
      image's own range, 0.5 being the reference's binarisation (utility/raw_data_process.py:105-106);
    * ``contact_span`` (default ``(4, 4)``) -- the extent of the image in taxel pitches, one number or (rows, columns);
    * the gain is ``HR_scale_num``: masses come out in the dataset's units, before ``_prep`` divided the target.

    A bad value raises ``TactileSRHipError`` here, before any launch."""
    try:
        gain = float(config.get("HR_scale_num", 1.0))
    except (TypeError, ValueError) as e:
        raise TactileSRHipError(f"HR_scale_num: {e}") from None
    return Fh.contact_readout_args(config.get("contact_threshold", 0.0), config.get("contact_threshold_mode", "abs"),
                                   gain, config.get("contact_span", (4, 4)))


class _ContactSums:
    """Whole-set sums of ``contact_iou``, ``contact_centroid_err`` and ``contact_mass_err`` for ``eval_func``: per value
    ``sum_b w_b v_b`` and ``sum_b w_b`` over the samples whose value is not NaN and whose weight is not 0, in fp64 on the
    device; one read-back at the end."""
    COLS = (2, 4, 5)                                              # IoU, centroid distance, relative mass error

    def __init__(self):
        self.tot = None

    def add(self, pair_raw, weight=None):
        v = pair_raw[:, list(self.COLS)].double()
        w = torch.ones(v.shape[0], dtype=torch.float64, device=v.device) if weight is None else weight.double()
        keep = ~torch.isnan(v) & (w != 0)[:, None]
        wk = torch.where(keep, w[:, None].expand_as(v), torch.zeros_like(v))
        part = torch.stack([(torch.where(keep, v, torch.zeros_like(v)) * wk).sum(0), wk.sum(0)])
        self.tot = part if self.tot is None else self.tot + part

    def means(self):
        if self.tot is None:
            return (float("nan"),) * 3
        num, den = self.tot.cpu().tolist()
        return tuple(n / d if d > 0 else float("nan") for n, d in zip(num, den))


def pixel_is_plain_mse(pixel) -> bool:
    """Whether a ``pixel_loss_config`` result is the reference's criterion: the step then issues the MSE launch."""
    return pixel[0] == "mse" and pixel[2] == 0


@dataclasses.dataclass(frozen=True)
class SRLossSpec(Fh.SRLossOptions):
    """The loss of the SR train step as the config states it, parsed once: ``functional.SRLossOptions`` (what the loss
    launches read) plus where the degradation term finds its inputs -- ``deg_gamma``, the config's scalar (``None``: the
    batch carries one), and ``deg_channel``, the channel of the prepared ``LR`` that holds the z-taxels.  With the
    degradation term off, ``deg_gamma``, ``deg_channel`` and ``deg_gain`` are ``None`` (``degradation_loss_config``).
    Hashable: ``GraphedTrainStep`` keys its capture on it."""
    deg_gamma: typing.Optional[float] = None
    deg_channel: typing.Optional[int] = None

    @classmethod
    def from_config(cls, config) -> "SRLossSpec":
        """From ``ssim_loss_config``, ``pixel_loss_config``, ``degradation_loss_config`` and ``sample_weight_config``: a
        value one of them refuses raises its ``TactileSRHipError`` here, before any launch."""
        ssim_weight, window, sigma, data_range = ssim_loss_config(config)
        pixel_kind, pixel_param, fg_weight, fg_threshold = pixel_loss_config(config)
        deg_weight, deg_gamma, deg_channel, deg_gain = degradation_loss_config(config)
        return cls(ssim_weight=ssim_weight, window=window, sigma=sigma, data_range=data_range, pixel_kind=pixel_kind,
                   pixel_param=pixel_param, fg_weight=fg_weight, fg_threshold=fg_threshold, deg_weight=deg_weight,
                   deg_gamma=deg_gamma, deg_channel=deg_channel, deg_gain=deg_gain,
                   sample_weight_norm=sample_weight_config(config))


def _degradation_gamma(spec, batch_gamma):
    """The gamma the degradation launch takes: the batch's own, else the config scalar; ``None`` with the term off;
    refused when a non-zero weight has neither.  Both steps call it before the forward, so the refusal precedes every
    launch."""
    if spec.deg_weight == 0:
        return None
    if batch_gamma is not None:
        return batch_gamma
    if spec.deg_gamma is None:
        raise TactileSRHipError("degradation_loss_weight is non-zero but there is no degradation_gamma key and the batch "
                                "carries no gamma")
    return spec.deg_gamma


def sr_loss_report(spec, terms):
    """The report dict of a train step from the ``functional.SRLossTerms`` of its loss -- the one rule of the eager and
    the graph-captured step.  ``total_loss`` always; the pixel term under ``mse_loss`` (the plain MSE) or ``pixel_loss``
    (any other pixel setting), unless the loss is the plain MSE with no other term and no weights; a configured criterion
    alone reports the loss tensor itself as ``pixel_loss``.  With an SSIM term ``ssim``, the mean of the per-sample values
    -- with weights the weighted mean ``(1/B) sum_b s_b ssim_b``, one more ``functional.weighted_mean`` launch; with a
    degradation term ``degradation_loss`` = ``mean_b q_b``; with weights ``labeled_weight``, the sum of the valid
    weights / B."""
    d = {"total_loss": terms.loss}
    alone = terms.ssim is None and terms.q is None and terms.scale is None
    if not (alone and spec.plain_mse):
        d["mse_loss" if spec.plain_mse else "pixel_loss"] = terms.loss if alone else terms.pixel
    if terms.scale is not None:
        d["labeled_weight"] = terms.stats[0] / terms.scale.shape[0]
    if terms.ssim is not None:
        d["ssim"] = terms.ssim.mean() if terms.scale is None else Fh.weighted_mean(terms.ssim, terms.scale)[0]
    if terms.q is not None:
        d["degradation_loss"] = terms.q.mean()
    return d


def sr_step_loss(spec, out, LR, HR, gamma, weight, *, autograd):
    """``(loss, dy or None, loss_dict)`` of one train step from the model's output ``out`` on the prepared ``LR`` / ``HR``:
    the loss of ``spec`` through ``functional.sr_loss_terms`` -- through autograd for the eager step (``dy`` is ``None``),
    outside it for the graph capture (``dy`` is the gradient the engine's backward takes) -- and ``sr_loss_report``'s dict.
    ``gamma`` is ``_degradation_gamma``'s result, ``weight`` the (B,) supervision weights or ``None``.  The z-taxels are
    ``LR[:, spec.deg_channel]``, detached and read in place."""
    deg_z = LR.detach()[:, spec.deg_channel] if spec.deg_weight != 0 else None
    terms = Fh.sr_loss_terms(out, HR, spec, deg_z, gamma, weight, autograd=autograd)
    return terms.loss, terms.dy, sr_loss_report(spec, terms)


def train_cal_loss(model, batch, config):
    """``total_loss`` is always in the dict.  With an SSIM term it also holds ``ssim`` and the pixel term, under
    ``mse_loss`` when that is the plain MSE; under any other pixel setting the term is reported as ``pixel_loss``.

    With a non-zero ``degradation_loss_weight`` (``degradation_loss_config``) the loss gains
    ``weight * mean_b q_b`` and the dict ``degradation_loss`` (that mean) and the pixel term under its usual key.  The
    z-taxels are the prepared ``LR[:, degradation_channel]``, detached: the term sends no gradient to ``LR``
    (``LR.grad`` holds what the pixel and SSIM terms send through the model, nothing from the residual's own
    ``d q / d z``).  A batch may be ``(LR, HR, gamma)`` with a (B,) per-sample ``gamma``, which overrides
    ``degradation_gamma``; without the key, or with weight 0, the step is unchanged.

    A batch may be ``(LR, HR, gamma, weight)`` (``gamma`` may be ``None``) with (B,) supervision weights ``w_b >= 0``:
    the pixel and SSIM terms count sample ``b`` with the scale ``s_b`` of ``functional.sample_scale`` under the config's
    ``sample_weight_norm`` (``sample_weight_config``), the degradation term keeps counting every sample, and the ``HR``
    of a sample with ``w_b = 0`` is never read by the loss (it may hold anything).  The dict then holds the weighted
    pixel term ``(1/B) sum_b s_b pix_b`` under its usual key, the weighted ``ssim`` ``(1/B) sum_b s_b ssim_b`` with an
    SSIM term, ``labeled_weight`` (the sum of the valid weights / B) and ``degradation_loss`` with that term; the plain
    MSE setting runs the per-sample launch with kind ``"mse"``.

    Every setting takes one path: the config is parsed once into an ``SRLossSpec``, and ``sr_step_loss`` -- which the
    capture of ``GraphedTrainStep`` calls too -- issues the launches of ``functional.sr_loss_fwd_bwd`` through one
    autograd function and builds the dict by the rule of ``sr_loss_report``.  The configured ``degradation_gain`` reaches
    the launch as parsed whatever the batch form (0.0 means 0)."""
    device = next(model.parameters()).device
    spec = SRLossSpec.from_config(config)
    weight = _batch_weight(batch, device)
    gamma = _degradation_gamma(spec, _batch_gamma(batch, device) if spec.deg_weight != 0 else None)   # read with the term on
    LR, HR = _prep(batch, config, device)
    loss, _, loss_dict = sr_step_loss(spec, model(LR), LR, HR, gamma, weight, autograd=True)
    return loss, loss_dict


def fused_clip_applies(model, optimizer) -> bool:
    """Whether ``optimizer.step_clipped`` clips exactly what the reference clips: the optimizer is
    ``tactilesr_amd.optim.Adam`` and the model parameters with a gradient are, by identity, the parameters it steps
    (those of its groups with a gradient).  Host-only."""
    from ..optim import Adam
    if not isinstance(optimizer, Adam):
        return False
    have = {id(p) for p in model.parameters() if p.grad is not None}
    stepped = {id(p) for g in optimizer.param_groups for p in g["params"] if p.grad is not None}
    return have == stepped


def train_one_iter(model, optimizer, batch, config, grad_sync=None, check_finite=False, cur_iter=None,
                   clip_grad_norm=0.0, ema=None):
    """zero_grad -> backward -> step, the order of cpu/trainer.py:352-361.  ``grad_sync`` (optional)
    is called between backward and step (data-parallel gradient averaging: tactilesr_amd.ddp).

    ``clip_grad_norm > 0`` clips the gradients to that global L2 norm before the step, after ``grad_sync`` (the
    reference ``Trainer(clip_grad_norm=...)``, cpu/trainer.py:354-356: ``clip_grad_norm_(model.parameters(), c)``);
    ``<= 0``, the default, leaves the step as it is.  With ``tactilesr_amd.optim.Adam`` stepping exactly the model's
    parameters that have a gradient, the clip is fused into the step (``Adam.step_clipped``: a norm kernel, then the
    Adam launch scales the gradients); otherwise -- another optimizer, or one that holds only part of them (the Seqs
    transplant, train/tactileSRSeqs_train.py:74-77) -- the reference's own two calls run:
    ``torch.nn.utils.clip_grad_norm_(model.parameters(), c)``, then ``optimizer.step()``.

    ``check_finite=True`` reproduces the reference trainer's per-iteration failure check
    (``Trainer._log_iter_metrics``, cpu/trainer.py:259,280-284): the loss is read back (a host sync, like the
    reference's ``loss.detach().cpu().item()``) and a NaN / Inf raises ``FloatingPointError`` with the reference's
    message.  Off by default so that a step enqueues without a device round trip."""
    if grad_sync is not None and hasattr(grad_sync, "pre_forward"):
        grad_sync.pre_forward()          # broadcast_buffers=True: rank 0's BatchNorm statistics, like torch DDP
    losses, loss_dict = train_cal_loss(model, batch, config)
    optimizer.zero_grad()
    losses.backward()
    if grad_sync is not None:
        grad_sync()
    if clip_grad_norm > 0:
        if fused_clip_applies(model, optimizer):
            optimizer.step_clipped(clip_grad_norm)
        else:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad_norm)
            optimizer.step()
    else:
        optimizer.step()
    if ema is not None:
        ema.update()
    if check_finite:
        import math
        value = float(losses.detach())
        if not math.isfinite(value):
            raise FloatingPointError(f"Loss became infinite or NaN at iteration={cur_iter}! "
                                     f"loss_dict={ {k: float(v.detach()) for k, v in loss_dict.items()} }.")
    return loss_dict


@torch.no_grad()
def eval_func(model, test_loader, config, windowed_ssim=False, self_ensemble=None, ema=None, taxel_noise=None,
              noise_seed=0, *, contact=False, degradation=False):
    """The reference's three averages (loss, SSIM, PSNR).  ``windowed_ssim=True`` appends a fourth: the windowed SSIM
    of ``functional.ssim`` with the config's ``ssim_window`` / ``ssim_sigma`` / ``ssim_data_range`` (``ssim_loss_config``),
    averaged the same way; the first three are unchanged.

    ``self_ensemble`` (``None``, the default: one forward per batch, the results unchanged) names an op set of
    ``functional.self_ensemble`` -- ``"dihedral"``, ``"rot90"`` or a tuple of ops -- and scores the mean of the model's
    outputs over those transforms of the taxels (plane by plane) instead.

    ``ema`` (a ``tactilesr_amd.WeightEMA`` of this model; ``None``, the default: the results unchanged) scores the
    averaged weights: the loop runs under ``ema.applied()`` and the model's own weights are back afterwards.

    ``taxel_noise`` (a ``functional.TaxelNoise`` or a dict of its fields; ``None``, the default: the results unchanged)
    scores the model on degraded taxels: after ``_prep`` each batch's ``LR`` passes through one
    ``functional.taxel_noise`` launch with seed ``noise_seed``, offset 0 and ``id_base`` = the number of samples seen so
    far, so sample ``k`` of the set always meets the same noise -- the score is deterministic and does not depend on the
    loader's batch size (beyond the averaging over batches itself).  It composes with ``self_ensemble`` and ``ema``.

    ``degradation=True`` (default ``False``: the results unchanged) appends one more value, after the windowed SSIM when
    that is on: the batch-averaged ``mean_b q_b`` of ``functional.degradation_fwd_bwd`` between the output pooled onto
    the taxels and the (noisy, when ``taxel_noise`` is on) z-taxels the model saw -- a score that needs no HR.  It reads
    ``degradation_gamma`` / ``degradation_channel`` / ``degradation_gain`` of ``degradation_loss_config`` whatever the
    weight; a 3-tuple batch's per-sample ``gamma`` overrides the key.

    Batches that carry a weight (4-tuples) turn the loss, SSIM, PSNR and windowed SSIM into
    ``sum_b w_b m_b / sum_b w_b`` over the whole set, from the per-sample values (``functional.pixel_loss_per_sample``,
    ``psnr_ssim``, ``ssim``) through ``functional.weighted_mean``: a sample with ``w_b = 0`` stays out even when its
    metric is NaN (its ``HR`` may hold anything), and a set whose weights sum to 0 returns NaN for these averages.  The
    degradation score stays the plain mean over all samples.  Without weights the results are unchanged.

    ``contact=True`` (default ``False``: the returned tuple unchanged, bit for bit) appends three values after every
    other one: ``contact_iou``, ``contact_centroid_err`` (taxel pitches) and ``contact_mass_err`` (relative), from one
    ``functional.contact_metrics`` launch per batch on ``(out, HR)`` with the keys of ``contact_readout_config``.  They
    are sample means over the whole set, ``sum_b v_b / #valid`` -- not means of batch means -- in which a sample whose
    value is NaN (no contact on one side) is left out of that value; a value with no valid sample is NaN.  With weighted
    batches they are ``sum_b w_b v_b / sum_b w_b`` over the valid samples with ``w_b != 0``.  It composes with
    ``self_ensemble``, ``ema``, ``taxel_noise`` and ``degradation``.

    ``contact`` and ``degradation`` are passed by keyword."""
    if ema is not None:
        with ema.applied():
            return eval_func(model, test_loader, config, windowed_ssim, self_ensemble, None, taxel_noise, noise_seed,
                             contact=contact, degradation=degradation)
    con = contact_readout_config(config) if contact else None
    con_sums = _ContactSums() if contact else None
    # the SSIM window and, for the degradation score (read whatever the configured weight), gamma / channel / gain
    spec = SRLossSpec.from_config({**config, "degradation_loss_weight": 1.0} if degradation else config)
    tot_deg = 0.0
    noise = Fh.taxel_noise_spec(taxel_noise)
    seen = 0
    device = next(model.parameters()).device
    model.eval()
    tot_loss = tot_ssim = tot_psnr = tot_wssim = 0.0
    n = 0
    window, sigma, data_range = spec.window, spec.sigma, spec.data_range
    weighted = None             # whether the set's batches carry weights: all of them or none
    tot_w = 0.0
    for batch in test_loader:
        LR, HR = _prep(batch, config, device)
        if noise is not None:
            LR = Fh.taxel_noise(LR, noise, noise_seed, 0, id_base=seen)
            seen += LR.shape[0]
        out = model(LR) if self_ensemble is None else Fh.self_ensemble(model, LR.contiguous(), self_ensemble)
        sw = _batch_weight(batch, device)
        if weighted is None:
            weighted = sw is not None
        elif weighted != (sw is not None):
            raise TactileSRHipError("eval_func: some batches of the set carry a weight and some do not")
        if sw is not None:       # sums of w_b m_b: the "batch" scale is w_b itself, and weighted_mean divides by B
            B = LR.shape[0]
            s, stats = Fh.sample_scale(sw, "batch")
            mse_b = Fh.pixel_loss_per_sample(out, HR, "mse", scale=s)[0]
            ps, ss = Fh.psnr_ssim(out, HR, config["sensorMaxVaule_factor"], reference_quirk=True)
            tot_loss += B * float(Fh.weighted_mean(mse_b, s))
            tot_psnr += B * float(Fh.weighted_mean(ps, s))
            tot_ssim += B * float(Fh.weighted_mean(ss, s))
            if windowed_ssim:
                tot_wssim += B * float(Fh.weighted_mean(Fh.ssim(out, HR, data_range, window, sigma), s))
            tot_w += float(stats[0])
        else:
            tot_loss += float(Fh.mse_loss(out, HR))
            ps, ss = Fh.psnr_ssim(out, HR, config["sensorMaxVaule_factor"], reference_quirk=True)
            tot_psnr += float(ps.mean())
            tot_ssim += float(ss.mean())
            if windowed_ssim:
                tot_wssim += float(Fh.ssim(out, HR, data_range, window, sigma).mean())
        if contact:
            con_sums.add(Fh.contact_metrics(out.float(), HR, *con)[0].raw, sw)
        if degradation:
            gamma = _degradation_gamma(spec, _batch_gamma(batch, device))
            tot_deg += float(Fh.degradation_fwd_bwd(out, LR[:, spec.deg_channel], gamma, spec.deg_gain, want_dy=False)[0].mean())
        n += 1
    if weighted:
        avg = (lambda v: v / tot_w) if tot_w > 0 else (lambda v: float("nan"))
        res = (avg(tot_loss), avg(tot_ssim), avg(tot_psnr))
        if windowed_ssim:
            res += (avg(tot_wssim),)
    else:
        res = (tot_loss / n, tot_ssim / n, tot_psnr / n)
        if windowed_ssim:
            res += (tot_wssim / n,)
    if degradation:
        res += (tot_deg / n,)
    if contact:
        res += con_sums.means()
    return res
