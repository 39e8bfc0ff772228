"""HIP-backed functional pieces of the SR training / eval step that sit outside the model:
target preparation, MSE loss, PSNR / SSIM, the differentiable SSIM and the MSE + SSIM loss (reference
train/tactileSR_train.py:41-51,66-101; utility/tools.py:49-114), and the pixel losses with a contact weight
(L1 / Charbonnier / Huber: not in the reference, whose criterion is nn.MSELoss), and the degradation-consistency term
(the SR output pooled back onto the taxels by the sensor model's masks, model/tPSFNet.py:129-141)."""
from __future__ import annotations

import ctypes
import dataclasses as _dc
import math as _math
import typing as _typing

import torch

from ._lib import call, ptr, stream, c_int as _I, c_float as _F, c_longlong as _L, c_double as _D, TactileSRHipError


def prepare_target(HR_raw: torch.Tensor, HR_scale_num: float = 10.0, scale_factor: int = 10) -> torch.Tensor:
    """``HR.float()/HR_scale_num`` + ``F.interpolate(HR, (4sf,4sf), bilinear)`` in one kernel
    (train/tactileSR_train.py:44-45)."""
    if not HR_raw.is_cuda:
        raise TactileSRHipError("prepare_target needs a ROCm tensor (no CPU fallback)")
    hr = HR_raw.detach().float().contiguous()
    B, C, hin, win = hr.shape
    assert C == 1
    H = W = 4 * scale_factor
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=hr.device)
    call("tsr_target_prep", ptr(hr), ptr(out), _F(1.0 / HR_scale_num), _I(B), _I(hin), _I(win), _I(H), _I(W), stream())
    return out


def mse_fwd_bwd(y: torch.Tensor, target: torch.Tensor):
    """``nn.MSELoss()(y, target)`` and its gradient w.r.t. ``y`` from one pass, outside autograd:
    (loss as a 1-element tensor, dy)."""
    y = y.contiguous()
    t = target.detach().float().contiguous()
    dy = torch.empty_like(y)
    loss = torch.empty(1, dtype=torch.float32, device=y.device)
    work = torch.empty(256, dtype=torch.float64, device=y.device)
    call("tsr_mse_fwd_bwd", ptr(y), ptr(t), ptr(dy), ptr(loss), _L(y.numel()), _F(1.0), ptr(work), stream())
    return loss, dy


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, target):
        loss, dy = mse_fwd_bwd(y, target)
        ctx.save_for_backward(dy)
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        (dy,) = ctx.saved_tensors
        return dy * gout, None


def mse_loss(y: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``nn.MSELoss()(y, target)`` (mean over all elements): loss and d loss/d y from one pass."""
    if not y.is_cuda:
        raise TactileSRHipError("mse_loss needs ROCm tensors (no CPU fallback)")
    return _MSE.apply(y.float(), target)


def _ssim_launch(y: torch.Tensor, t: torch.Tensor, data_range, window, sigma, K1, K2, dy, dy_scale, accumulate,
                 scale=None):
    """One ``tsr_ssim_fwd_bwd`` launch on contiguous fp32 (B,1,H,W) tensors: the per-sample values; ``dy`` (or None)
    is written / accumulated in place.  With ``scale`` (the (B,) fp32 device vector of ``sample_scale``) the launch is
    ``tsr_ssim_fwd_bwd_ps``: sample ``b``'s gradient is multiplied by ``scale[b]`` and a sample whose scale is 0 is
    skipped."""
    if y.dim() != 4 or y.shape[1] != 1 or t.shape != y.shape:
        raise TactileSRHipError(f"ssim needs two (B,1,H,W) tensors of one shape, got {tuple(y.shape)} and {tuple(t.shape)}")
    B, _, H, W = y.shape
    vals = torch.empty(B, dtype=torch.float32, device=y.device)
    if scale is not None:
        call("tsr_ssim_fwd_bwd_ps", ptr(y), ptr(t), _I(B), _I(H), _I(W), _I(int(window)), _D(float(sigma)),
             _D((K1 * data_range) ** 2), _D((K2 * data_range) ** 2), ptr(scale), ptr(vals), ptr(dy), _F(dy_scale),
             _I(accumulate), stream())
        return vals
    call("tsr_ssim_fwd_bwd", ptr(y), ptr(t), _I(B), _I(H), _I(W), _I(int(window)), _D(float(sigma)),
         _D((K1 * data_range) ** 2), _D((K2 * data_range) ** 2), ptr(vals), ptr(dy), _F(dy_scale), _I(accumulate),
         stream())
    return vals


def ssim(a: torch.Tensor, b: torch.Tensor, data_range: float = 1.0, window: int = 11, sigma: float = 1.5,
         K1: float = 0.01, K2: float = 0.03) -> torch.Tensor:
    """Per-sample SSIM of two (B,1,H,W) batches, no autograd.  ``window`` odd in 3..11: the Gaussian-windowed form
    (valid correlation, H, W <= 128); ``window=0``: one global window, the reference's ``calculationSSIM``
    (utility/tools.py:66-81) -- with ``data_range=1.0`` (C1 = 0.01^2, C2 = 0.03^2) what ``psnr_ssim`` reports."""
    if not a.is_cuda or not b.is_cuda:
        raise TactileSRHipError("ssim needs ROCm tensors (no CPU fallback)")
    return _ssim_launch(a.detach().float().contiguous(), b.detach().float().contiguous(), data_range, window, sigma,
                        K1, K2, None, 0.0, 0)


class _SSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, target, data_range, window, sigma, K1, K2):
        y = y.contiguous()
        t = target.detach().float().contiguous()
        dy = torch.empty_like(y)
        vals = _ssim_launch(y, t, data_range, window, sigma, K1, K2, dy, -1.0 / y.shape[0], 0)
        ctx.save_for_backward(dy)
        return 1.0 - vals.mean()

    @staticmethod
    def backward(ctx, gout):
        (dy,) = ctx.saved_tensors
        return dy * gout, None, None, None, None, None, None


def ssim_loss(y: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, window: int = 11, sigma: float = 1.5,
              K1: float = 0.01, K2: float = 0.03) -> torch.Tensor:
    """``1 - mean_b ssim_b`` (the reference's "# ssim loss", utility/tools.py:84-114, in the windowed or the global
    form of ``ssim``): value and d loss / d y from one launch; the target gets no gradient."""
    if not y.is_cuda or not target.is_cuda:
        raise TactileSRHipError("ssim_loss needs ROCm tensors (no CPU fallback)")
    return _SSIMLoss.apply(y.float(), target, data_range, window, sigma, K1, K2)


PIXEL_KINDS = {"mse": 0, "l1": 1, "charbonnier": 2, "huber": 3}
PIXEL_PARAM_DEFAULT = {"charbonnier": 1e-3, "huber": 1.0}       # eps, delta
PIXEL_LOSS_WORK = 2048                                          # TSR_PIXEL_LOSS_WORK of include/tactilesr_hip.h


def pixel_loss_args(kind="mse", param=None, fg_weight=0.0, fg_threshold=0.0):
    """``(kind, param, fg_weight, fg_threshold)`` as ``tsr_pixel_loss_fwd_bwd`` takes them -- the name lower-cased, the
    parameter's default filled in (eps = 1e-3 for ``"charbonnier"``, delta = 1.0 for ``"huber"``; ``None`` for the
    kinds that read none), floats -- or ``TactileSRHipError`` for an unknown name or a value the kernel would refuse.  Host-only."""
    name = str(kind).lower()
    if name not in PIXEL_KINDS:
        raise TactileSRHipError(f"pixel loss {kind!r} is not one of {sorted(PIXEL_KINDS)}")
    try:
        p = float(PIXEL_PARAM_DEFAULT[name] if param is None else param) if name in PIXEL_PARAM_DEFAULT else None
        w, thr = float(fg_weight), float(fg_threshold)
    except (TypeError, ValueError) as e:
        raise TactileSRHipError(f"pixel loss {name}: {e}") from None
    if p is not None and not (0 < p < float("inf")):
        raise TactileSRHipError(f"pixel loss {name} needs a finite parameter > 0, got {p}")
    if not (0 <= w < float("inf")):
        raise TactileSRHipError(f"the contact weight must be finite and >= 0, got {w}")
    if thr != thr:
        raise TactileSRHipError("the contact threshold is NaN")
    return name, p, w, thr


def pixel_loss_fwd_bwd(y: torch.Tensor, target: torch.Tensor, kind: str = "mse", param=None, fg_weight: float = 0.0,
                       fg_threshold: float = 0.0, dy=None, dy_scale: float = 1.0, accumulate: bool = False,
                       want_dt: bool = False):
    """``mean_p w_p rho(y_p - t_p)`` with ``rho`` the ``kind`` (``"mse"``, ``"l1"``, ``"charbonnier"``: ``param`` = eps,
    ``"huber"``: ``param`` = delta) and ``w_p = 1 + fg_weight * [t_p > fg_threshold]``, and its gradients, from one
    ``tsr_pixel_loss_fwd_bwd`` launch outside autograd: ``(loss (1,), dy)`` or, with ``want_dt``, ``(loss, dy, dt)``.
    ``dy = dy_scale * d loss / d y`` is a new tensor, or the given contiguous fp32 ``dy`` written in place
    (``accumulate=True``: added to it); ``dt = -dy_scale * d loss / d y`` is the gradient with respect to the target."""
    if not y.is_cuda or not target.is_cuda:
        raise TactileSRHipError("pixel_loss_fwd_bwd needs ROCm tensors (no CPU fallback)")
    name, p, w, thr = pixel_loss_args(kind, param, fg_weight, fg_threshold)
    y = y.detach().float().contiguous()
    t = target.detach().float().contiguous()
    if t.shape != y.shape:
        raise TactileSRHipError(f"pixel loss needs two tensors of one shape, got {tuple(y.shape)} and {tuple(t.shape)}")
    if dy is None:
        if accumulate:
            raise TactileSRHipError("pixel_loss_fwd_bwd: accumulate=True needs the dy to add to")
        dy = torch.empty_like(y)
    elif dy.dtype != torch.float32 or dy.shape != y.shape:
        raise TactileSRHipError("pixel_loss_fwd_bwd: dy must be an fp32 tensor of y's shape")
    dt = torch.empty_like(y) if want_dt else None
    loss = torch.empty(1, dtype=torch.float32, device=y.device)
    work = torch.empty(PIXEL_LOSS_WORK, dtype=torch.float64, device=y.device)
    call("tsr_pixel_loss_fwd_bwd", ptr(y), ptr(t), _L(y.numel()), _I(PIXEL_KINDS[name]), _D(0.0 if p is None else p), _F(w), _F(thr), ptr(loss),
         ptr(dy), _F(dy_scale), _I(1 if accumulate else 0), ptr(dt), ptr(work), stream())
    return (loss, dy, dt) if want_dt else (loss, dy)


class _PixelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, target, kind, param, fg_weight, fg_threshold):
        res = pixel_loss_fwd_bwd(y, target, kind, param, fg_weight, fg_threshold, want_dt=ctx.needs_input_grad[1])
        ctx.save_for_backward(*res[1:])
        return res[0][0]

    @staticmethod
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        return saved[0] * gout, (saved[1] * gout if len(saved) == 2 else None), None, None, None, None


def pixel_loss(y: torch.Tensor, target: torch.Tensor, kind: str = "mse", param=None, fg_weight: float = 0.0,
               fg_threshold: float = 0.0) -> torch.Tensor:
    """The autograd form of ``pixel_loss_fwd_bwd``: value and gradients from one launch.  ``y`` gets a gradient, and so
    does ``target`` when it requires one (the exact ``-d loss / d y``: the contact weight is not differentiated)."""
    if not y.is_cuda or not target.is_cuda:
        raise TactileSRHipError("pixel_loss needs ROCm tensors (no CPU fallback)")
    if target.requires_grad and target.dtype != torch.float32:
        raise TactileSRHipError("pixel_loss: a target that requires grad must be fp32")
    return _PixelLoss.apply(y.float(), target, kind, param, fg_weight, fg_threshold)


# ----------------------------------------------------------------------------------------------------------------------
# Per-sample supervision weights (tsr_sample_scale, tsr_pixel_loss_ps_fwd_bwd, tsr_ssim_fwd_bwd_ps, tsr_weighted_mean):
# sample b of a batch counts in the pixel and SSIM terms with a weight w_b >= 0; w_b = 0 is an unlabeled sample whose
# target is never read.
# ----------------------------------------------------------------------------------------------------------------------
SAMPLE_WEIGHT_NORMS = {"sum": 0, "batch": 1}
PIXEL_LOSS_PS_MAX_WGS = 2048                                    # TSR_PIXEL_LOSS_PS_MAX_WGS of include/tactilesr_hip.h


def sample_weight_norm_arg(norm="sum") -> str:
    """The normalisation mode as a key of ``SAMPLE_WEIGHT_NORMS``, or ``TactileSRHipError``.  Host-only."""
    name = str(norm).lower()
    if name not in SAMPLE_WEIGHT_NORMS:
        raise TactileSRHipError(f"sample_weight_norm {norm!r} is not one of {sorted(SAMPLE_WEIGHT_NORMS)}")
    return name


def _sample_vector(w, B: int, device, who: str, what: str = "sample weight") -> torch.Tensor:
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] != B:
        raise TactileSRHipError(f"{who}: the {what} is a ({B},) tensor, got "
                                f"{tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")
    if not w.is_cuda or w.device != device:
        raise TactileSRHipError(f"{who}: the {what} must be on the ROCm device of the images (no CPU fallback)")
    return w.detach().float().contiguous()


def sample_scale(w: torch.Tensor, norm: str = "sum"):
    """``(s (B,), stats (2,))`` of a (B,) device weight vector from one ``tsr_sample_scale`` launch.  A weight is valid
    when it is finite and >= 0.  ``norm="sum"``: ``s_b = w_b * B / D`` with ``D`` the fp64 sum of the valid weights (0
    when ``D == 0``), so a term ``(1/B) sum_b s_b x_b`` is the mean of ``x`` over the labeled weight; ``norm="batch"``:
    ``s_b = w_b``, the divisor stays ``B`` (the mode whose average over data-parallel ranks is exact).  An invalid
    weight gives ``s_b = NaN`` and is left out of ``D``.  ``stats = (D, number of valid weights > 0)``."""
    mode = SAMPLE_WEIGHT_NORMS[sample_weight_norm_arg(norm)]
    if not isinstance(w, torch.Tensor) or not w.is_cuda:
        raise TactileSRHipError("sample_scale needs a ROCm tensor (no CPU fallback)")
    w = _sample_vector(w, w.shape[0] if w.dim() == 1 else -1, w.device, "sample_scale")
    B = w.shape[0]
    if B == 0:
        raise TactileSRHipError("sample_scale: an empty weight vector")
    s = torch.empty(B, dtype=torch.float32, device=w.device)
    stats = torch.empty(2, dtype=torch.float32, device=w.device)
    call("tsr_sample_scale", ptr(w), _I(B), _I(mode), ptr(s), ptr(stats), stream())
    return s, stats


def weighted_mean(v: torch.Tensor, scale=None) -> torch.Tensor:
    """``(1/B) sum_{scale_b != 0} scale_b v_b`` as a (1,) tensor from one ``tsr_weighted_mean`` launch (fp64, index
    order, one rounding); ``scale=None``: the plain mean.  An entry whose scale is 0 is not read: a NaN there stays out."""
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dim() != 1 or v.shape[0] == 0:
        raise TactileSRHipError("weighted_mean needs a non-empty (B,) ROCm tensor (no CPU fallback)")
    v = v.detach().float().contiguous()
    if scale is not None:
        scale = _sample_vector(scale, v.shape[0], v.device, "weighted_mean", "scale")
    out = torch.empty(1, dtype=torch.float32, device=v.device)
    call("tsr_weighted_mean", ptr(v), ptr(scale), _I(v.shape[0]), ptr(out), stream())
    return out


def pixel_loss_per_sample(y: torch.Tensor, target: torch.Tensor, kind: str = "mse", param=None, fg_weight: float = 0.0,
                          fg_threshold: float = 0.0, scale=None, dy=None, dy_scale: float = 1.0, accumulate: bool = False,
                          want_dt: bool = False, max_wgs=None):
    """The per-sample form of ``pixel_loss_fwd_bwd`` from one ``tsr_pixel_loss_ps_fwd_bwd`` launch, outside autograd:
    ``(pix (B,), dy)`` or, with ``want_dt``, ``(pix, dy, dt)``.  ``pix_b`` is sample ``b``'s own mean over its
    ``P = numel / B`` elements (not multiplied by its scale).  ``dy = dy_scale * scale_b * d pix_b / d y / B``: with
    ``scale=None`` (all ones) the gradient of ``mean_b pix_b``, bit for bit ``pixel_loss_fwd_bwd``'s.  ``scale`` is the
    (B,) device vector of ``sample_scale``; a sample whose scale is 0 is skipped -- its ``y`` and ``target`` are not
    read, its ``pix`` is 0, its ``dy`` rows are 0 (untouched with ``accumulate=True``) and its ``dt`` rows 0.
    ``max_wgs`` caps the grid (the result does not depend on it)."""
    if not y.is_cuda or not target.is_cuda:
        raise TactileSRHipError("pixel_loss_per_sample needs ROCm tensors (no CPU fallback)")
    name, p, w, thr = pixel_loss_args(kind, param, fg_weight, fg_threshold)
    y = y.detach().float().contiguous()
    t = target.detach().float().contiguous()
    if t.shape != y.shape or y.dim() < 1 or y.numel() == 0:
        raise TactileSRHipError(f"pixel loss needs two non-empty tensors of one shape, got {tuple(y.shape)} and "
                                f"{tuple(t.shape)}")
    B = y.shape[0]
    if scale is not None:
        scale = _sample_vector(scale, B, y.device, "pixel_loss_per_sample", "scale")
    if dy is None:
        if accumulate:
            raise TactileSRHipError("pixel_loss_per_sample: accumulate=True needs the dy to add to")
        dy = torch.empty_like(y)
    elif dy.dtype != torch.float32 or dy.shape != y.shape:
        raise TactileSRHipError("pixel_loss_per_sample: dy must be an fp32 tensor of y's shape")
    dt = torch.empty_like(y) if want_dt else None
    pix = torch.empty(B, dtype=torch.float32, device=y.device)
    args = [ptr(y), ptr(t), _I(B), _L(y.numel() // B), _I(PIXEL_KINDS[name]), _D(0.0 if p is None else p), _F(w), _F(thr),
            ptr(scale), ptr(pix), ptr(dy), _F(dy_scale), _I(1 if accumulate else 0), ptr(dt)]
    if max_wgs is None:
        call("tsr_pixel_loss_ps_fwd_bwd", *args, stream())
    else:
        call("tsr_pixel_loss_ps_fwd_bwd_wgs", *args, _I(int(max_wgs)), stream())
    return (pix, dy, dt) if want_dt else (pix, dy)



# ----------------------------------------------------------------------------------------------------------------------
# Degradation consistency (tsr_degrade_fwd_bwd, csrc/degrade_loss.hip): the image pooled onto the 4x4 taxels by the
# sensor model's masks (reference model/tPSFNet.py:129-141 at 100x100), against the measured z-taxels.
# ----------------------------------------------------------------------------------------------------------------------
DEGRADE_MAX_HW = 128
DEGRADE_MAX_WGS = 2048                                          # TSR_DEGRADE_MAX_WGS of include/tactilesr_hip.h
DEGRADE_GAMMA_MAX = 1e6                                         # TSR_DEGRADE_GAMMA_MAX: beyond it the masks are flat


def degrade_gamma_arg(gamma, B: int, device=None):
    """``(gamma_dev tensor or None, gamma_all float)`` as ``tsr_degrade_fwd_bwd`` takes them: a float in (0, 1e6] for
    every image, or a ``(B,)`` tensor on the device (made fp32 and contiguous; its values are checked by the kernel,
    which answers a bad one with an all-NaN image).  ``TactileSRHipError`` otherwise.  Host-only for a float."""
    if isinstance(gamma, torch.Tensor):
        if gamma.dim() == 0 and not gamma.is_cuda:
            gamma = float(gamma)
        else:
            if gamma.dim() != 1 or gamma.shape[0] != B:
                raise TactileSRHipError(f"a gamma tensor must have shape ({B},), got {tuple(gamma.shape)}")
            if device is not None and gamma.device != device:
                raise TactileSRHipError(f"the gamma tensor is on {gamma.device}, the image on {device}")
            return gamma.detach().float().contiguous(), 0.0
    try:
        g = float(gamma)
    except (TypeError, ValueError) as e:
        raise TactileSRHipError(f"degradation gamma: {e}") from None
    if not (0 < g <= DEGRADE_GAMMA_MAX):
        raise TactileSRHipError(f"the degradation gamma must be in (0, {DEGRADE_GAMMA_MAX:g}], got {g}")
    return None, g


def _degrade_gain(gain) -> float:
    try:
        g = float(gain)
    except (TypeError, ValueError) as e:
        raise TactileSRHipError(f"degradation gain: {e}") from None
    if not _math.isfinite(g):
        raise TactileSRHipError(f"the degradation gain must be finite, got {g}")
    return g


def _degrade_image(y: torch.Tensor, who: str) -> torch.Tensor:
    if not y.is_cuda:
        raise TactileSRHipError(f"{who} needs ROCm tensors (no CPU fallback)")
    if y.dim() != 4 or y.shape[1] != 1 or not (1 <= y.shape[2] <= DEGRADE_MAX_HW and 1 <= y.shape[3] <= DEGRADE_MAX_HW):
        raise TactileSRHipError(f"{who} needs a (B,1,H,W) image with 1 <= H, W <= {DEGRADE_MAX_HW}, got {tuple(y.shape)}")
    return y.detach().float().contiguous()


def _degrade_taxels(z: torch.Tensor, B: int, device, who: str):
    """``(tensor to pass, z_bstride)`` of the taxels ``z`` -- (B,16), (B,4,4), (B,1,4,4) or a channel slice
    ``LR[:, c]`` / ``LR[:, c:c+1]`` of a contiguous (B,C,4,4) fp32 tensor, which is passed in place."""
    if z.device != device:
        raise TactileSRHipError(f"{who}: the taxels are on {z.device}, the image on {device}")
    if z.shape[0] != B or z.numel() != 16 * B:
        raise TactileSRHipError(f"{who} needs 16 taxels per image, got {tuple(z.shape)} for {B} images")
    z = z.detach()
    zz = z.reshape(B, 16) if z.dim() == 2 else z.reshape(B, 4, 4) if z.shape[-2:] == (4, 4) else None
    if zz is None:
        raise TactileSRHipError(f"{who}: taxels of shape {tuple(z.shape)} are not (B,16) or (B,[1,]4,4)")
    inner = (1,) if zz.dim() == 2 else (4, 1)
    if zz.dtype == torch.float32 and tuple(zz.stride()[1:]) == inner and (B == 1 or zz.stride(0) >= 16):
        return zz, (16 if B == 1 else zz.stride(0))
    return zz.float().contiguous(), 16


def _degrade_launch(y, z, z_bstride, gamma, gain, lr_deg, q, dy, dy_scale, accumulate, dz, max_wgs=None):
    B, _, H, W = y.shape
    gdev, gall = degrade_gamma_arg(gamma, B, y.device)
    args = [ptr(y), _I(B), _I(H), _I(W), ctypes.c_void_p(z.data_ptr()) if z is not None else ptr(None), _L(z_bstride),
            ptr(gdev), _D(gall), _D(_degrade_gain(gain)), ptr(lr_deg), ptr(q), ptr(dy), _F(dy_scale),
            _I(1 if accumulate else 0), ptr(dz)]
    if max_wgs is None:
        call("tsr_degrade_fwd_bwd", *args, stream())
    else:
        call("tsr_degrade_fwd_bwd_wgs", *args, _I(int(max_wgs)), stream())


def degrade(y: torch.Tensor, gamma, gain: float = 1.0) -> torch.Tensor:
    """The sensor model's pooling of a (B,1,H,W) image onto the taxels, (B,1,4,4), no autograd: at 100x100 with
    ``gain=1`` the reference's ``degradation_process`` (model/tPSFNet.py:129-141); on another grid the same masks
    sampled at the pixel centres of ``F.interpolate(align_corners=False)``.  ``gamma`` (the mask width, ``alphaBeta[2]``)
    is a float or a (B,) device tensor; ``gain`` multiplies the result (it undoes a ``/HR_scale_num`` of the image)."""
    y = _degrade_image(y, "degrade")
    out = torch.empty(y.shape[0], 1, 4, 4, dtype=torch.float32, device=y.device)
    _degrade_launch(y, None, 0, gamma, gain, out, None, None, 0.0, False, None)
    return out


def degradation_fwd_bwd(y: torch.Tensor, z: torch.Tensor, gamma, gain: float = 1.0, dy=None, dy_scale: float = 1.0,
                        accumulate: bool = False, want_dz: bool = False, want_dy: bool = True):
    """``q_b = mean_ac (degrade(y)_b - z_b)^2`` per image and its gradients from one ``tsr_degrade_fwd_bwd`` launch,
    outside autograd: ``(q (B,), lr_deg (B,1,4,4), dy)`` or, with ``want_dz``, ``(q, lr_deg, dy, dz (B,1,4,4))``.
    ``dy = dy_scale * d q_b / d y`` is a new tensor, or the given contiguous fp32 ``dy`` written in place
    (``accumulate=True``: added to it); ``dz = dy_scale * d q_b / d z``.  ``z`` is (B,16), (B,4,4), (B,1,4,4) or a channel
    slice of a contiguous (B,C,4,4) fp32 tensor (read in place).  ``gamma`` is not differentiated.  ``want_dy=False``
    (a score: ``eval_func``) passes no ``dy`` to the launch, which then neither allocates nor writes one, and returns
    ``None`` in its place; the other outputs keep their bits."""
    y = _degrade_image(y, "degradation_fwd_bwd")
    B = y.shape[0]
    zz, zs = _degrade_taxels(z, B, y.device, "degradation_fwd_bwd")
    if not want_dy:
        if dy is not None or accumulate:
            raise TactileSRHipError("degradation_fwd_bwd: want_dy=False takes no dy and no accumulate")
    elif dy is None:
        if accumulate:
            raise TactileSRHipError("degradation_fwd_bwd: accumulate=True needs the dy to add to")
        dy = torch.empty_like(y)
    elif dy.dtype != torch.float32 or dy.shape != y.shape or not dy.is_cuda or not dy.is_contiguous():
        raise TactileSRHipError("degradation_fwd_bwd: dy must be a contiguous fp32 ROCm tensor of y's shape")
    lr_deg = torch.empty(B, 1, 4, 4, dtype=torch.float32, device=y.device)
    q = torch.empty(B, dtype=torch.float32, device=y.device)
    dz = torch.empty(B, 1, 4, 4, dtype=torch.float32, device=y.device) if want_dz else None
    _degrade_launch(y, zz, zs, gamma, gain, lr_deg, q, dy, dy_scale, accumulate, dz)
    return (q, lr_deg, dy, dz) if want_dz else (q, lr_deg, dy)


class _DegradationLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, z, gamma, gain):
        want_dz = ctx.needs_input_grad[1]
        res = degradation_fwd_bwd(y, z, gamma, gain, dy_scale=1.0 / y.shape[0], want_dz=want_dz)
        ctx.save_for_backward(*res[2:])
        ctx.z_shape = z.shape
        return res[0].mean()

    @staticmethod
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        dz = (saved[1] * gout).reshape(ctx.z_shape) if len(saved) == 2 else None
        return saved[0] * gout, dz, None, None


def degradation_loss(y: torch.Tensor, z: torch.Tensor, gamma, gain: float = 1.0) -> torch.Tensor:
    """The autograd form of ``degradation_fwd_bwd``: ``mean_b q_b``, value and gradients from one launch.  ``y`` gets a
    gradient, and so does ``z`` when it requires one; ``gamma`` never does."""
    if not y.is_cuda or not z.is_cuda:
        raise TactileSRHipError("degradation_loss needs ROCm tensors (no CPU fallback)")
    if z.requires_grad and z.dtype != torch.float32:
        raise TactileSRHipError("degradation_loss: taxels that require grad must be fp32")
    return _DegradationLoss.apply(y.float(), z, gamma, gain)


@_dc.dataclass(frozen=True)
class SRLossOptions:
    """The constants of the SR training loss under ``sr_loss_fwd_bwd``'s names and defaults; the tensors of a call
    (``deg_z``, ``deg_gamma``, ``sample_weight``) travel beside it.  Hashable.  ``deg_gain`` is read only with a
    non-zero ``deg_weight``."""
    ssim_weight: float = 0.0
    data_range: float = 1.0
    window: int = 11
    sigma: float = 1.5
    K1: float = 0.01
    K2: float = 0.03
    pixel_kind: str = "mse"
    pixel_param: _typing.Optional[float] = None
    fg_weight: float = 0.0
    fg_threshold: float = 0.0
    deg_weight: float = 0.0
    deg_gain: _typing.Optional[float] = 1.0
    sample_weight_norm: str = "sum"

    @property
    def plain_mse(self) -> bool:
        """The reference's criterion, nn.MSELoss: the pixel term is then the MSE launch."""
        return str(self.pixel_kind).lower() == "mse" and float(self.fg_weight) == 0


class SRLossTerms(_typing.NamedTuple):
    """What one evaluation of the SR loss gives; ``None`` where a term is absent.  ``pixel`` is the pixel term (the
    weighted one with weights), ``ssim`` and ``q`` the per-sample values of the SSIM and degradation terms, ``pix_b``,
    ``scale`` and ``stats`` the per-sample pixel values and ``sample_scale``'s two results of a weighted batch.  ``dy``
    is ``None`` in the autograd form."""
    loss: torch.Tensor
    dy: _typing.Optional[torch.Tensor]
    pixel: torch.Tensor
    ssim: _typing.Optional[torch.Tensor]
    q: _typing.Optional[torch.Tensor]
    pix_b: _typing.Optional[torch.Tensor]
    scale: _typing.Optional[torch.Tensor]
    stats: _typing.Optional[torch.Tensor]


def _optional_terms(t: SRLossTerms) -> tuple:
    """The tail of the variable-length returns of ``sr_loss_fwd_bwd(return_parts=True)`` and ``sr_loss``."""
    return ((t.q,) if t.q is not None else ()) + ((t.pix_b, t.scale, t.stats) if t.scale is not None else ())


def _sr_loss_launches(y, target, o: SRLossOptions, deg_z, deg_gamma, sample_weight, parts: bool = True) -> SRLossTerms:
    """Every launch of the SR loss, in the order of ``sr_loss_fwd_bwd``'s docstring; ``loss`` and ``pixel`` are (1,)
    tensors.  ``parts=False`` leaves out the one launch that only a report needs (the weighted pixel term beside an SSIM
    term): ``pixel`` is then the loss before the degradation term."""
    if not y.is_cuda or not target.is_cuda:
        raise TactileSRHipError("sr_loss_fwd_bwd needs ROCm tensors (no CPU fallback)")
    lam, lam_d = float(o.ssim_weight), float(o.deg_weight)
    if lam_d != 0 and (deg_z is None or deg_gamma is None):
        raise TactileSRHipError("sr_loss_fwd_bwd: a non-zero deg_weight needs deg_z and deg_gamma")
    B = y.shape[0]
    s = stats = pix_b = vals = q = None
    if sample_weight is not None:
        s, stats = sample_scale(_sample_vector(sample_weight, B, y.device, "sr_loss_fwd_bwd"), o.sample_weight_norm)
        pix_b, dy = pixel_loss_per_sample(y, target, o.pixel_kind, o.pixel_param, o.fg_weight, o.fg_threshold, scale=s)
    elif o.plain_mse:
        pix, dy = mse_fwd_bwd(y, target)
    else:
        pix, dy = pixel_loss_fwd_bwd(y, target, o.pixel_kind, o.pixel_param, o.fg_weight, o.fg_threshold)
    if lam != 0:
        vals = _ssim_launch(y.contiguous(), target.detach().float().contiguous(), o.data_range, o.window, o.sigma, o.K1, o.K2,
                            dy, -lam / B, 1, scale=s)
    if lam_d != 0:
        q = degradation_fwd_bwd(y, deg_z, deg_gamma, o.deg_gain, dy=dy, dy_scale=lam_d / B, accumulate=True)[0]
    if s is None:
        loss = pix if vals is None else pix + lam * (1.0 - vals.mean())
    else:
        loss = pix = weighted_mean(pix_b if vals is None else pix_b + lam * (1.0 - vals), s)
        if vals is not None and parts:
            pix = weighted_mean(pix_b, s)
    if q is not None:
        loss = loss + lam_d * q.mean()
    return SRLossTerms(loss, dy, pix, vals, q, pix_b, s, stats)


def sr_loss_fwd_bwd(y: torch.Tensor, target: torch.Tensor, ssim_weight: float = 0.0, data_range: float = 1.0,
                    window: int = 11, sigma: float = 1.5, K1: float = 0.01, K2: float = 0.03, return_parts: bool = False,
                    pixel_kind: str = "mse", pixel_param=None, fg_weight: float = 0.0, fg_threshold: float = 0.0,
                    sample_weight=None, sample_weight_norm: str = "sum",
                    deg_weight: float = 0.0, deg_z=None, deg_gamma=None, deg_gain: float = 1.0):
    """``pixel(y, target) + ssim_weight * (1 - mean_b ssim_b) + deg_weight * mean_b q_b`` and its gradient w.r.t. ``y``,
    outside autograd: ``(loss (1,), dy)``.  The pixel launch, then the SSIM launch accumulating
    ``-ssim_weight / B * d ssim_b / d y`` into the same ``dy``, then the degradation launch (``degradation_fwd_bwd`` on
    the taxels ``deg_z`` with ``deg_gamma`` and ``deg_gain``) accumulating ``deg_weight / B * d q_b / d y``.  The pixel
    term is the MSE launch (``mse_fwd_bwd``) for ``pixel_kind="mse"`` with ``fg_weight == 0``, otherwise
    ``pixel_loss_fwd_bwd`` with the four pixel arguments; ``ssim_weight == 0`` and ``deg_weight == 0`` is that launch
    alone, launch for launch, and ``deg_weight == 0`` issues exactly the launches it issued before the term existed.
    ``return_parts=True`` appends the terms: ``(loss, dy, pixel (1,), ssim (B,) or None)`` and, with a non-zero
    ``deg_weight``, ``q (B,)`` as a fifth.

    ``sample_weight`` (default ``None``: exactly the launches above) is a (B,) device tensor of supervision weights
    ``w_b >= 0``.  With ``s = sample_scale(sample_weight, sample_weight_norm)`` the loss is
    ``(1/B) sum_{s_b != 0} s_b [pix_b + ssim_weight (1 - ssim_b)] + deg_weight * mean_b q_b``: the pixel and SSIM terms
    count sample ``b`` with ``s_b``, the degradation term keeps counting every sample, and the target of a sample with
    ``w_b = 0`` is never read (it may hold NaN).  The launches are then: the scale launch, the per-sample pixel launch
    (``pixel_loss_per_sample``, the plain MSE as kind ``"mse"``), the SSIM launch in its ``_ps`` form accumulating, the
    unchanged degradation launch, and the weighted means (``weighted_mean``).  ``return_parts`` reports the weighted
    pixel term ``(1/B) sum s_b pix_b`` as ``pixel`` and appends three more: the per-sample ``pix (B,)``, ``s (B,)`` and
    the ``stats (2,)`` of ``sample_scale``."""
    t = _sr_loss_launches(y, target, SRLossOptions(ssim_weight, data_range, window, sigma, K1, K2, pixel_kind, pixel_param,
                                                   fg_weight, fg_threshold, deg_weight, deg_gain, sample_weight_norm),
                          deg_z, deg_gamma, sample_weight, parts=return_parts)
    return (t.loss, t.dy, t.pixel, t.ssim) + _optional_terms(t) if return_parts else (t.loss, t.dy)


class _SRLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, target, deg_z, deg_gamma, sample_weight, opts):
        t = _sr_loss_launches(y, target, opts, deg_z, deg_gamma, sample_weight)
        ctx.save_for_backward(t.dy)
        t = t._replace(loss=t.loss[0], dy=None, pixel=t.pixel[0])
        ctx.mark_non_differentiable(*(v for v in t[1:] if v is not None))      # everything but the loss is a report
        return tuple(t)

    @staticmethod
    def backward(ctx, gout, *_gparts):
        (dy,) = ctx.saved_tensors
        return dy * gout, None, None, None, None, None


def sr_loss_terms(y: torch.Tensor, target: torch.Tensor, opts: SRLossOptions, deg_z=None, deg_gamma=None, sample_weight=None,
                  *, autograd: bool) -> SRLossTerms:
    """The SR loss of ``sr_loss_fwd_bwd`` under the options ``opts`` (any object with ``SRLossOptions``'s attributes), with
    ``loss`` and ``pixel`` as scalars.  ``autograd=True``: ``loss`` carries the gradient to ``y`` (nothing else gets
    one) and ``dy`` is ``None``; ``autograd=False``: outside autograd, ``dy`` is the gradient.  The launches are the
    same in both forms."""
    if autograd:
        return SRLossTerms(*_SRLoss.apply(y.float(), target, None if deg_z is None else deg_z.detach(), deg_gamma,
                                          None if sample_weight is None else sample_weight.detach(), opts))
    t = _sr_loss_launches(y.float(), target, opts, deg_z, deg_gamma, sample_weight)
    return t._replace(loss=t.loss[0], pixel=t.pixel[0])


def sr_loss(y: torch.Tensor, target: torch.Tensor, ssim_weight: float, data_range: float = 1.0, window: int = 11,
            sigma: float = 1.5, pixel_kind: str = "mse", pixel_param=None, fg_weight: float = 0.0,
            fg_threshold: float = 0.0, sample_weight=None, sample_weight_norm: str = "sum", deg_weight: float = 0.0,
            deg_z=None, deg_gamma=None, deg_gain: float = 1.0):
    """The autograd form of ``sr_loss_fwd_bwd``, a thin adapter over ``sr_loss_terms``:
    ``(loss, pixel term, per-sample ssim)`` and, with a non-zero ``deg_weight``, the per-sample ``q`` as a fourth
    (``ssim`` is then ``None`` when ``ssim_weight == 0``); only ``loss`` carries a gradient (to ``y`` -- the taxels
    ``deg_z`` get none here: ``degradation_loss`` is the form that differentiates them).  With ``sample_weight`` (any
    ``ssim_weight`` and ``deg_weight``, zero included) the weighted loss of ``sr_loss_fwd_bwd``; the tuple then ends
    with the per-sample ``pix (B,)``, the scale ``s (B,)`` and ``stats (2,)``, and its pixel term is the weighted one."""
    t = sr_loss_terms(y, target, SRLossOptions(ssim_weight, data_range, window, sigma, pixel_kind=pixel_kind,
                                               pixel_param=pixel_param, fg_weight=fg_weight, fg_threshold=fg_threshold,
                                               deg_weight=deg_weight, deg_gain=deg_gain,
                                               sample_weight_norm=sample_weight_norm),
                      deg_z, deg_gamma, sample_weight, autograd=True)
    return (t.loss, t.pixel, t.ssim) + _optional_terms(t)


def psnr_ssim(a: torch.Tensor, b: torch.Tensor, maxValue: float, reference_quirk: bool = True,
              C1: float = 0.01 ** 2, C2: float = 0.03 ** 2):
    """Per-sample ``calculationPSNR`` / ``calculationSSIM`` for (B,1,H,W) batches.  With
    ``reference_quirk`` the squared error is divided by shape[0]*shape[1] of the (1,H,W) slice the
    reference's eval_func passes (= H, not H*W; utility/tools.py:60-61, train/tactileSR_train.py:89)."""
    a = a.detach().float().contiguous()
    b = b.detach().float().contiguous()
    B, H, W = a.shape[0], a.shape[-2], a.shape[-1]
    n = a.numel() // B
    div = float(1 * H) if reference_quirk else float(H * W)
    ps = torch.empty(B, dtype=torch.float32, device=a.device)
    ss = torch.empty(B, dtype=torch.float32, device=a.device)
    call("tsr_psnr_ssim", ptr(a), ptr(b), _I(B), _I(n), _D(div), _D(maxValue), _D(C1), _D(C2), ptr(ps), ptr(ss), stream())
    return ps, ss


# ----------------------------------------------------------------------------------------------------------------------
# Rot90 / flip augmentation and the geometric self-ensemble (tsr_gather_dihedral, csrc/dihedral.hip).  A data path: none
# of it is differentiable, and nothing here builds an autograd graph.
# ----------------------------------------------------------------------------------------------------------------------
DIHEDRAL_SETS = {"rot90": (0, 1, 2, 3), "dihedral": (0, 1, 2, 3, 4, 5, 6, 7)}
AXIS_MODES = ("planes", "vector")


def _dihedral_parts(op: int):
    """``(transpose, flip source rows, flip source columns)`` of op = k + 4 f: output (i, j) is the source element
    ``(a(u), b(v))`` with ``(u, v) = (j, i)`` under a transpose."""
    return bool(op & 1), bool(op & 2), bool(bin(op).count("1") & 1)


def _dihedral_coord(op: int, i: int, j: int, n: int):
    tr, fr, fc = _dihedral_parts(op)
    u, v = (j, i) if tr else (i, j)
    return (n - 1 - u if fr else u), (n - 1 - v if fc else v)


def _dihedral_tables():
    n = 3
    maps = [tuple(_dihedral_coord(op, i, j, n) for i in range(n) for j in range(n)) for op in range(8)]
    comp = [[0] * 8 for _ in range(8)]
    for a in range(8):
        for b in range(8):
            # D_b(D_a(x)): element (i, j) of the result is element D_b-coordinate of D_a(x), itself a D_a-coordinate of x
            both = tuple(_dihedral_coord(a, *_dihedral_coord(b, i, j, n), n) for i in range(n) for j in range(n))
            comp[a][b] = maps.index(both)
    inv = [comp[a].index(0) for a in range(8)]
    return comp, inv


_DIHEDRAL_COMPOSE, _DIHEDRAL_INVERSE = _dihedral_tables()


def _check_op(op) -> int:
    o = int(op)
    if o != op or not 0 <= o <= 7:
        raise TactileSRHipError(f"a dihedral op is an integer in 0..7 (k + 4 f), got {op!r}")
    return o


def dihedral_compose(a: int, b: int) -> int:
    """The op c with ``D_c(x) = D_b(D_a(x))``: ``a`` first, then ``b``.  Host-only integer table."""
    return _DIHEDRAL_COMPOSE[_check_op(a)][_check_op(b)]


def dihedral_inverse(op: int) -> int:
    """The op that undoes ``op``: ``dihedral_compose(op, dihedral_inverse(op)) == 0``.  Host-only integer table."""
    return _DIHEDRAL_INVERSE[_check_op(op)]


def dihedral_ops(spec) -> tuple:
    """``"rot90"`` -> ops 0..3 (the reference's augmentData), ``"dihedral"`` -> ops 0..7, or an explicit non-empty
    sequence of distinct ops, as a tuple."""
    if isinstance(spec, str):
        if spec not in DIHEDRAL_SETS:
            raise TactileSRHipError(f"op set {spec!r} is not one of {sorted(DIHEDRAL_SETS)} or a tuple of ops")
        return DIHEDRAL_SETS[spec]
    try:
        ops = tuple(_check_op(o) for o in spec)
    except TypeError:
        raise TactileSRHipError(f"op set {spec!r} is not one of {sorted(DIHEDRAL_SETS)} or a tuple of ops") from None
    if not ops or len(set(ops)) != len(ops):
        raise TactileSRHipError(f"an op set needs at least one op and no repeats, got {ops}")
    return ops


def dihedral_op_mask(ops) -> int:
    m = 0
    for o in ops:
        m |= 1 << _check_op(o)
    return m


def dihedral_axis_tables(C: int, axis_cnt: int = 3):
    """``(cmap (8, C) int32, csign (8, C) float32)`` of ``axis_mode="vector"``, CPU tensors.  Within each group of
    ``axis_cnt`` channels, channel 0 is the force along +H (rows), channel 1 the force along +W and channel 2 (and any
    further one) a scalar such as the normal force (the layout sketched in utility/raw_data_process.py:134-141).  The
    pair (0, 1) transforms with the op's 2x2 coordinate matrix -- a mirror or a turn also turns the in-plane force --
    and the other channels never change.  Output plane c is ``csign[op][c] * D_op(plane cmap[op][c])``."""
    C, axis_cnt = int(C), int(axis_cnt)
    if axis_cnt < 2 or C <= 0 or C % axis_cnt:
        raise TactileSRHipError(f"vector axis mode needs C a positive multiple of axis_cnt >= 2, got C={C}, axis_cnt={axis_cnt}")
    cmap = torch.arange(C, dtype=torch.int32).repeat(8, 1)
    csign = torch.ones(8, C, dtype=torch.float32)
    for op in range(8):
        tr, fr, fc = _dihedral_parts(op)
        sr, sc = (-1.0 if fr else 1.0), (-1.0 if fc else 1.0)
        for g in range(0, C, axis_cnt):
            # source (r, c) lands at i = sr r, j = sc c, or under a transpose at i = sc c, j = sr r
            cmap[op, g], cmap[op, g + 1] = (g + 1, g) if tr else (g, g + 1)
            csign[op, g], csign[op, g + 1] = (sc, sr) if tr else (sr, sc)
    return cmap, csign


def _dihedral_plane_torch(x: torch.Tensor, op: int) -> torch.Tensor:
    if op & 4:
        x = x.flip(-1)
    return torch.rot90(x, op & 3, (-2, -1))


def _dihedral_torch(x, ops, index, out, scale, accumulate, tables, op_all):
    """The transform composed from torch ops (index_select, flip, rot90): CPU tensors and dtypes other than fp32."""
    n_out = x.shape[0] if index is None else int(index.shape[0])
    src = x if index is None else x.index_select(0, index.to(x.device).long())
    op_list = [int(op_all)] * n_out if ops is None else [int(o) for o in torch.as_tensor(ops).tolist()]
    if len(op_list) != n_out:
        raise TactileSRHipError(f"dihedral: {len(op_list)} ops for {n_out} output samples")
    res = torch.empty_like(src)
    for op in sorted(set(op_list)):
        _check_op(op)
        sel = torch.tensor([k for k, o in enumerate(op_list) if o == op], dtype=torch.long, device=x.device)
        part = src.index_select(0, sel)
        if tables is not None:
            cmap, csign = tables
            part = part.index_select(1, cmap[op].to(x.device).long())
            neg = (csign[op] < 0).to(x.device).view(1, -1, 1, 1)
            part = torch.where(neg, -part, part)
        res.index_copy_(0, sel, _dihedral_plane_torch(part, op))
    if scale == 1.0 and not accumulate:
        val = res
    elif not accumulate:
        val = res * scale
    else:
        val = (out.double() + float(scale) * res.double()).to(res.dtype)
    if out is None:
        return val.contiguous()
    out.copy_(val)
    return out


def _memory_overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Whether two tensors of one device touch a common byte: the byte ranges of contiguous tensors, else (a strided
    view) whether they share a storage."""
    if a.device != b.device or a.numel() == 0 or b.numel() == 0:
        return False
    if a.is_contiguous() and b.is_contiguous():
        a0, b0 = a.data_ptr(), b.data_ptr()
        return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def dihedral(x: torch.Tensor, ops=None, index=None, out=None, scale: float = 1.0, accumulate: bool = False,
             axis_mode: str = "planes", op_all: int = 0, *, op_mask=None, axis_cnt: int = 3, tables=None) -> torch.Tensor:
    """``out[b] = (accumulate ? out[b] : 0) + scale * D_{ops[b]}(x[index[b]])``: gather and rot90 / flip in one
    ``tsr_gather_dihedral`` launch.  ``x`` is ``(N, C, H, W)`` or ``(N, H, W)``; ``ops`` an int32 tensor (or a sequence)
    of one op per output sample, ``None`` = ``op_all`` for all; ``index`` an int64 tensor (or a sequence), ``None`` = the
    identity; ``out``, when given, must not overlap ``x`` in memory (the kernel reads while it writes).  An
    op is ``k + 4 f``: mirror along W when ``f``, then ``np.rot90(x, k, axes=(-2, -1))``.  ``axis_mode="planes"``
    transforms every plane on its own (the reference); ``"vector"`` also maps the in-plane force channels
    (``dihedral_axis_tables(C, axis_cnt)``).  Keyword-only, beyond the reference-shaped arguments: ``tables`` passes device
    copies of those tables made once (the loader does), ``axis_cnt`` their group size, and ``op_mask`` (default: every op
    the shape admits, or ``op_all`` alone) is the set of ops the launch accepts: a sample with any other op, or with an
    index outside ``x``, comes out all-NaN, never as an out-of-range access.  No host synchronisation on a ROCm fp32
    tensor.  A CPU tensor or another dtype takes a torch-composed path with the same results (it reads ``ops`` on the
    host and raises on a bad op).  Not differentiable: a data path, run it outside autograd."""
    if axis_mode not in AXIS_MODES:
        raise TactileSRHipError(f"axis_mode {axis_mode!r} is not one of {AXIS_MODES}")
    if x.dim() == 3:
        res = dihedral(x.unsqueeze(1), ops, index, None if out is None else out.unsqueeze(1), scale, accumulate,
                       axis_mode, op_all, op_mask=op_mask, axis_cnt=axis_cnt, tables=tables)
        return res.squeeze(1)
    if x.dim() != 4:
        raise TactileSRHipError(f"dihedral needs (N,C,H,W) or (N,H,W), got {tuple(x.shape)}")
    x = x.detach()
    n_src, C, H, W = x.shape
    if index is not None:
        index = torch.as_tensor(index, device=x.device).to(torch.int64).contiguous()
        if index.dim() != 1:
            raise TactileSRHipError(f"dihedral: index must be one-dimensional, got {tuple(index.shape)}")
    B = n_src if index is None else int(index.shape[0])
    if accumulate and out is None:
        raise TactileSRHipError("dihedral: accumulate=True needs the out to add to")
    if out is not None and (tuple(out.shape) != (B, C, H, W) or out.dtype != x.dtype or out.device != x.device):
        raise TactileSRHipError("dihedral: out must have shape (B,C,H,W), and x's dtype and device")
    if out is not None and _memory_overlaps(x, out):
        raise TactileSRHipError("dihedral: out overlaps x in memory; the transform is not done in place")
    if axis_mode == "vector" and tables is None:
        tables = tuple(t.to(x.device) for t in dihedral_axis_tables(C, axis_cnt))
    elif axis_mode == "planes":
        tables = None
    if not x.is_cuda or x.dtype != torch.float32:
        return _dihedral_torch(x, ops, index, out, float(scale), bool(accumulate), tables, op_all)
    x = x.contiguous()
    if ops is not None:
        ops = torch.as_tensor(ops, device=x.device).to(torch.int32).contiguous()
        if ops.shape != (B,):
            raise TactileSRHipError(f"dihedral: ops must hold one op per output sample ({B}), got {tuple(ops.shape)}")
    if op_mask is None:
        op_mask = (1 << _check_op(op_all)) if ops is None else (0xff if H == W else 0x55)
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    elif not out.is_contiguous():
        raise TactileSRHipError("dihedral: out must be contiguous")
    cmap, csign = tables if tables is not None else (None, None)
    call("tsr_gather_dihedral", ptr(x), _I(n_src), ptr(index), ptr(ops), _I(int(op_all)), _I(int(op_mask)), ptr(cmap),
         ptr(csign), ptr(out), _I(B), _I(C), _I(H), _I(W), _F(float(scale)), _I(1 if accumulate else 0), stream())
    return out


@torch.no_grad()
def self_ensemble(model, LR: torch.Tensor, ops="dihedral", axis_mode: str = "planes") -> torch.Tensor:
    """Geometric self-ensemble: the mean over ``ops`` of ``D_op^-1(model(D_op(LR)))``, in eval mode and under
    ``no_grad`` (the model's training flag is restored).  For each op the whole batch is transformed with ``op_all``,
    the model runs, and ``(1/n) D_op^-1(y)`` is accumulated by the kernel's ``accumulate`` form: one rounding of the
    first term (none when 1/n is a power of two) and one fma per further term.  ``ops``: ``"dihedral"`` (8),
    ``"rot90"`` (4) or a tuple; ``ops=(0,)`` is ``model(LR)`` bit for bit.  ``axis_mode`` applies to ``LR``; the
    output is an image and is turned back plane by plane.  Not differentiable."""
    ops = dihedral_ops(ops)
    was_training = model.training
    model.eval()
    try:
        acc, w = None, 1.0 / len(ops)
        for op in ops:
            y = model(dihedral(LR, op_all=op, axis_mode=axis_mode))
            if acc is None:
                acc = dihedral(y, op_all=dihedral_inverse(op), scale=w)
            else:
                dihedral(y, op_all=dihedral_inverse(op), out=acc, scale=w, accumulate=True)
    finally:
        model.train(was_training)
    return acc


# ----------------------------------------------------------------------------------------------------------------------
# Taxel sensor noise (tsr_taxel_noise, csrc/taxel_noise.hip): gain drift, heteroscedastic Gaussian noise and dead taxels in
# one launch from a counter-based generator.  A data path like `dihedral`: not differentiable, no autograd graph.
# ----------------------------------------------------------------------------------------------------------------------
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TAXEL_NOISE_TAGS = {"noise": 0, "gain": 1, "dropout": 2}


def _f32(v) -> float:
    import numpy as np
    return float(np.float32(v))


@_dc.dataclass(frozen=True)
class TaxelNoise:
    """The degradation of ``taxel_noise`` (formulas: include/tactilesr_hip.h).  ``sigma_add`` / ``sigma_mul`` are a scalar
    or one value per axis (``axis_cnt`` of them; channel ``c`` is axis ``c % axis_cnt``): the noise of an element ``v`` has
    standard deviation ``sqrt(sigma_add^2 + (sigma_mul v)^2)``.  ``gain_jitter`` scales every physical taxel (shared by the
    frames of a sample) by a factor uniform in ``1 +- gain_jitter``; ``drop_prob`` is the share of dead taxels, which read
    ``drop_value`` in every channel.  Frozen; validated on construction (``TactileSRHipError``); the values are held as the
    fp32 numbers the kernel receives."""
    sigma_add: object = 0.0
    sigma_mul: object = 0.0
    gain_jitter: float = 0.0
    drop_prob: float = 0.0
    drop_value: float = 0.0
    axis_cnt: int = 3

    def __post_init__(self):
        a = self.axis_cnt
        if isinstance(a, bool) or not isinstance(a, int) or not 1 <= a <= 4:
            raise TactileSRHipError(f"TaxelNoise: axis_cnt must be an integer in 1..4, got {a!r}")

        def sig(name, v):
            try:
                vals = tuple(_f32(s) for s in v) if hasattr(v, "__len__") else (_f32(v),) * a
            except (TypeError, ValueError):
                raise TactileSRHipError(f"TaxelNoise: {name} must be a number or {a} numbers, got {v!r}") from None
            if len(vals) != a:
                raise TactileSRHipError(f"TaxelNoise: {name} needs one value or one per axis ({a}), got {len(vals)}")
            if not all(_math.isfinite(s) and s >= 0.0 for s in vals):
                raise TactileSRHipError(f"TaxelNoise: {name} must be finite and >= 0, got {vals}")
            return vals
        object.__setattr__(self, "sigma_add", sig("sigma_add", self.sigma_add))
        object.__setattr__(self, "sigma_mul", sig("sigma_mul", self.sigma_mul))
        for name in ("gain_jitter", "drop_prob", "drop_value"):
            try:
                v = _f32(getattr(self, name)) if name != "drop_prob" else float(getattr(self, name))
            except (TypeError, ValueError):
                raise TactileSRHipError(f"TaxelNoise: {name} must be a number, got {getattr(self, name)!r}") from None
            if not _math.isfinite(v):
                raise TactileSRHipError(f"TaxelNoise: {name} must be finite, got {v}")
            object.__setattr__(self, name, v)
        if not 0.0 <= self.drop_prob <= 1.0:
            raise TactileSRHipError(f"TaxelNoise: drop_prob must lie in [0, 1], got {self.drop_prob}")

    @property
    def drop_thresh(self) -> int:
        """``round(drop_prob 2^24)``: a taxel is dead when the top 24 bits of its word are below it."""
        return int(_math.floor(self.drop_prob * (1 << 24) + 0.5))

    @property
    def is_identity(self) -> bool:
        """Every effect neutral: the launch copies ``x`` bit for bit."""
        return (self.gain_jitter == 0.0 and self.drop_thresh == 0
                and all(s == 0.0 for s in self.sigma_add + self.sigma_mul))


def taxel_noise_spec(obj):
    """A ``TaxelNoise`` from a ``TaxelNoise`` (itself), a dict of its fields, or ``None`` (stays ``None``: no noise)."""
    if obj is None or isinstance(obj, TaxelNoise):
        return obj
    if isinstance(obj, dict):
        try:
            return TaxelNoise(**obj)
        except TypeError as e:
            raise TactileSRHipError(f"taxel noise spec: {e}") from None
    raise TactileSRHipError(f"a taxel noise spec is a TaxelNoise, a dict of its fields or None, got {type(obj).__name__}")


def _philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable uint64 arrays holding 32-bit values: the four output words, as uint64."""
    import numpy as np
    m32 = np.uint64(0xffffffff)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & m32, (k1 + np.uint64(_PHILOX_W1)) & m32
    return c0, c1, c2, c3


def _taxel_words_np(ids, blocks, tag, seed, offset):
    """(B, 4 blocks) uint32 words of effect ``tag`` for the sample ids (a numpy int64 array; bad ids are the caller's)."""
    import numpy as np
    j = np.arange(blocks, dtype=np.uint64)[None, :]
    i = np.asarray(ids).astype(np.uint64)[:, None]
    seed = int(seed) & 0xffffffffffffffff
    w = _philox_np(j, i, np.uint64(offset), np.uint64(tag), seed & 0xffffffff, seed >> 32)
    return np.stack(np.broadcast_arrays(*w), -1).reshape(len(ids), 4 * blocks).astype(np.uint32)


def _cossinpi_f32(a):
    """cos(pi a), sin(pi a) for fp32 ``a`` in [0, 2) on a grid of 2^-23: the quarter is taken off exactly, so the argument
    of cos / sin carries one rounding of pi r with |r| <= 1/4."""
    import numpy as np
    k = np.floor(a * np.float32(2.0) + np.float32(0.5))
    r = (a - k * np.float32(0.5)).astype(np.float32)
    t = np.float32(np.pi) * r
    c, s = np.cos(t), np.sin(t)
    q = k.astype(np.int64) & 3
    return (np.choose(q, [c, -s, -c, s]).astype(np.float32), np.choose(q, [s, c, -s, -c]).astype(np.float32))


def _taxel_noise_np(x, spec: TaxelNoise, seed, offset, ids):
    """The fp32 restatement of csrc/taxel_noise.hip in numpy (CPU tensors): the same Philox stream and formulas; an fma is
    taken in fp64 and rounded.  Within a few ulp of the device, not bit-equal (libm's logf / cos / sin)."""
    import numpy as np
    B, C, H, W = x.shape
    P, a = H * W, spec.axis_cnt
    f32 = np.float32
    ids = np.asarray(ids, dtype=np.int64)
    bad = (ids < 0) | (ids > 0x7fffffff)
    safe = np.where(bad, 0, ids)
    v = x.reshape(B, C // a, a, P).copy()
    two24 = f32(2.0 ** -24)
    if spec.gain_jitter != 0.0:
        w = _taxel_words_np(safe, (a * P + 3) // 4, 1, seed, offset)[:, :a * P].reshape(B, 1, a, P)
        u2m1 = f32(2.0) * ((w >> 8).astype(f32) * two24) - f32(1.0)
        g = (1.0 + np.float64(f32(spec.gain_jitter)) * u2m1.astype(np.float64)).astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            v = (g * v).astype(f32)
    active = np.array([spec.sigma_add[k] != 0.0 or spec.sigma_mul[k] != 0.0 for k in range(a)])
    if active.any():
        nb = (C * P + 3) // 4
        w = _taxel_words_np(safe, nb, 0, seed, offset).reshape(B, nb, 2, 2)
        u1 = (f32(2.0) * (w[..., 0] >> 9).astype(f32) + f32(1.0)) * two24
        a2 = (w[..., 1] >> 8).astype(f32) * f32(2.0 ** -23)
        R = np.sqrt(f32(-2.0) * np.log(u1)).astype(f32)
        c, s = _cossinpi_f32(a2)
        n = np.stack([R * c, R * s], -1).astype(f32).reshape(B, 4 * nb)[:, :C * P].reshape(B, C // a, a, P)
        sa = np.asarray(spec.sigma_add, f32).reshape(1, 1, a, 1)
        sm = np.asarray(spec.sigma_mul, f32).reshape(1, 1, a, 1)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (sm * v).astype(f32)
            sd = np.sqrt((t.astype(np.float64) * t + (sa * sa).astype(np.float64)).astype(f32))
            y = (v.astype(np.float64) + sd.astype(np.float64) * n).astype(f32)
        v = np.where(active.reshape(1, 1, a, 1), y, v)
    v = v.reshape(B, C, P)
    if spec.drop_thresh != 0:
        w = _taxel_words_np(safe, (P + 3) // 4, 2, seed, offset)[:, :P]
        v = np.where(((w >> 8) < np.uint32(spec.drop_thresh))[:, None, :], f32(spec.drop_value), v)
    v = np.ascontiguousarray(v, dtype=f32)
    if bad.any():
        v.view(np.uint32)[bad] = 0x7fc00000
    return v.reshape(B, C, H, W)


def _rng_words(seed, offset):
    seed, offset = int(seed) & 0xffffffffffffffff, int(offset)
    if not 0 <= offset <= 0xffffffff:
        raise TactileSRHipError(f"taxel noise: offset must lie in [0, 2^32), got {offset}")
    return seed, offset


def taxel_noise_rng(seed: int = 0, offset: int = 0, device="cuda") -> torch.Tensor:
    """The four int32 words ``{seed_lo, seed_hi, offset, 0}`` of ``taxel_noise(rng=...)`` on ``device``.  Rewrite word 2
    (``rng[2] = new_offset``, or ``copy_`` from a host tensor) between the replays of a captured graph."""
    seed, offset = _rng_words(seed, offset)
    import numpy as np
    return torch.from_numpy(np.array([seed & 0xffffffff, seed >> 32, offset, 0], dtype=np.uint32).view(np.int32)).to(device)


def taxel_noise(x: torch.Tensor, spec, seed: int = 0, offset: int = 0, ids=None, id_base: int = 0, out=None,
                rng=None) -> torch.Tensor:
    """Degrade the taxels ``x`` ``(B, C, H, W)`` fp32 with ``spec`` (a ``TaxelNoise``, a dict of its fields, or ``None`` =
    the identity) in one ``tsr_taxel_noise`` launch: gain drift, then Gaussian noise, then dead taxels (formulas:
    ``TaxelNoise`` and include/tactilesr_hip.h).  The draws come from Philox4x32-10 with key ``seed`` (64 bits; a larger or
    negative value is taken modulo 2^64) and counter ``(block, id, offset, tag)``: the noise of a sample is a pure function
    of ``(seed, offset, id, element)``.  ``id`` is ``ids[b]`` (an int64 tensor or a sequence) or ``id_base + b``; an id
    outside ``[0, 2^31)`` gives an all-NaN sample.  ``out`` may be ``x`` itself (in place) or a disjoint tensor.  ``rng`` -- a
    device int32 / uint32 tensor of the 4 words ``{seed_lo, seed_hi, offset, 0}`` (``taxel_noise_rng``) -- replaces
    ``seed`` / ``offset`` and is read by the kernel (``tsr_taxel_noise_dev``), so a captured graph draws fresh noise on each
    replay after the offset word is rewritten.  No host synchronisation on a ROCm tensor.  A CPU tensor runs a numpy fp32
    restatement of the same stream and formulas (within a few ulp of the device, not bit-equal).  Not differentiable: a
    data path, it carries no autograd graph."""
    spec = taxel_noise_spec(spec) or TaxelNoise()
    if x.dim() != 4:
        raise TactileSRHipError(f"taxel_noise needs (B,C,H,W), got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TactileSRHipError(f"taxel_noise needs fp32 taxels, got {x.dtype}")
    x = x.detach()
    B, C, H, W = x.shape
    if B == 0 or C == 0 or H == 0 or W == 0:
        raise TactileSRHipError(f"taxel_noise: an empty tensor {tuple(x.shape)}")
    if C % spec.axis_cnt:
        raise TactileSRHipError(f"taxel_noise: {C} channels are no multiple of axis_cnt = {spec.axis_cnt}")
    seed, offset = _rng_words(seed, offset)
    if ids is not None:
        ids = torch.as_tensor(ids, device=x.device).to(torch.int64).contiguous()
        if ids.shape != (B,):
            raise TactileSRHipError(f"taxel_noise: ids must hold one id per sample ({B}), got {tuple(ids.shape)}")
    if rng is not None:
        if (not isinstance(rng, torch.Tensor) or rng.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                or rng.numel() != 4 or rng.device != x.device or not rng.is_contiguous()):
            raise TactileSRHipError("taxel_noise: rng must be a contiguous int32 / uint32 tensor of 4 words on x's device")
    if out is not None:
        if tuple(out.shape) != (B, C, H, W) or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise TactileSRHipError("taxel_noise: out must be contiguous with x's shape, dtype and device")
        same = x.is_contiguous() and out.data_ptr() == x.data_ptr()
        if not same and _memory_overlaps(x, out):
            raise TactileSRHipError("taxel_noise: out overlaps x in memory without being x")
    if not x.is_cuda:
        import numpy as np
        if rng is not None:
            w = rng.view(torch.int32).numpy().view(np.uint32)
            seed, offset = int(w[0]) | (int(w[1]) << 32), int(w[2])
        idn = ids.numpy() if ids is not None else np.arange(B, dtype=np.int64) + int(id_base)
        res = torch.from_numpy(_taxel_noise_np(x.contiguous().numpy(), spec, seed, offset, idn))
        if out is None:
            return res
        out.copy_(res)
        return out
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    n = spec.axis_cnt
    sa, sm = (ctypes.c_float * n)(*spec.sigma_add), (ctypes.c_float * n)(*spec.sigma_mul)
    head = (ptr(x), ptr(out), _I(B), _I(C), _I(H), _I(W), _I(n), ctypes.cast(sa, ctypes.c_void_p),
            ctypes.cast(sm, ctypes.c_void_p), _F(spec.gain_jitter), _I(spec.drop_thresh), _F(spec.drop_value), ptr(ids),
            _L(int(id_base)))
    if rng is not None:
        call("tsr_taxel_noise_dev", *head, ptr(rng), stream())
    else:
        call("tsr_taxel_noise", *head, ctypes.c_ulonglong(seed), ctypes.c_uint(offset), stream())
    return out


def taxel_noise_bits(B: int, blocks: int, tag: int, seed: int = 0, offset: int = 0, ids=None, id_base: int = 0,
                     device="cuda") -> torch.Tensor:
    """The raw Philox stream of ``taxel_noise``: an int32 tensor ``(B, blocks, 4)`` holding the bit patterns of the words of
    blocks ``0 .. blocks - 1`` of effect ``tag`` (0 noise, 1 gain, 2 dropout) for samples ``ids[b]`` or ``id_base + b``
    (``tsr_taxel_noise_bits``; numpy on ``device="cpu"``).  A sample with an id outside ``[0, 2^31)`` holds 0x7fc00000."""
    B, blocks, tag = int(B), int(blocks), int(tag)
    if B <= 0 or blocks <= 0 or not 0 <= tag <= 0x7fffffff:
        raise TactileSRHipError(f"taxel_noise_bits: B and blocks must be positive and tag in [0, 2^31), got {B}, {blocks}, {tag}")
    seed, offset = _rng_words(seed, offset)
    dev = torch.device(device)
    if ids is not None:
        ids = torch.as_tensor(ids, device=dev).to(torch.int64).contiguous()
        if ids.shape != (B,):
            raise TactileSRHipError(f"taxel_noise_bits: ids must hold one id per sample ({B}), got {tuple(ids.shape)}")
    if dev.type != "cuda":
        import numpy as np
        idn = ids.numpy() if ids is not None else np.arange(B, dtype=np.int64) + int(id_base)
        bad = (idn < 0) | (idn > 0x7fffffff)
        w = _taxel_words_np(np.where(bad, 0, idn), blocks, tag, seed, offset)
        w[bad] = 0x7fc00000
        return torch.from_numpy(w.view(np.int32).reshape(B, blocks, 4).copy())
    out = torch.empty(B, blocks, 4, dtype=torch.int32, device=dev)
    call("tsr_taxel_noise_bits", ptr(out), _I(B), _I(blocks), ptr(ids), _L(int(id_base)), _I(tag), ctypes.c_ulonglong(seed),
         ctypes.c_uint(offset), stream())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Contact readout (tsr_contact_readout, csrc/contact_readout.hip): the geometry of the contact region of a pressure image
# and the overlap / error metrics of a pair, from one launch.  A readout: not differentiable, no autograd graph.
# ----------------------------------------------------------------------------------------------------------------------
CONTACT_REC = 16                                                # TSR_CONTACT_REC of include/tactilesr_hip.h
CONTACT_PAIR = 8                                                # TSR_CONTACT_PAIR
CONTACT_MAX_WGS = 2048                                          # TSR_CONTACT_MAX_WGS
CONTACT_MAX_PIXELS = 1 << 24                                    # counts stay exact in fp32
CONTACT_MODES = {"abs": 0, "range": 1}


class ContactReadout(_typing.NamedTuple):
    """One contact per image, in taxel-pitch units (``u`` along rows, ``v`` along columns; with ``span = 4`` taxel ``a``'s
    centre is at ``a``).  ``moments`` is ``(muu, mvv, muv)``; ``major`` / ``minor`` are the roots of the eigenvalues of
    that matrix; ``raw`` is the (B,16) record of ``tsr_contact_readout`` the other fields are views of."""
    count: torch.Tensor
    area: torch.Tensor
    mass: torch.Tensor
    total: torch.Tensor
    peak: torch.Tensor
    peak_pos: torch.Tensor
    centroid: torch.Tensor
    moments: torch.Tensor
    angle: torch.Tensor
    major: torch.Tensor
    minor: torch.Tensor
    tau: torch.Tensor
    raw: torch.Tensor


class ContactMetrics(_typing.NamedTuple):
    """The pair record of ``tsr_contact_readout``: ``raw`` is (B,8), the other fields are its columns."""
    inter: torch.Tensor
    union: torch.Tensor
    iou: torch.Tensor
    dice: torch.Tensor
    centroid_dist: torch.Tensor
    mass_rel_err: torch.Tensor
    peak_dist: torch.Tensor
    angle_diff: torch.Tensor
    raw: torch.Tensor


def _contact_readout_of(raw: torch.Tensor) -> ContactReadout:
    return ContactReadout(raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 4], raw[:, 5:7], raw[:, 7:9], raw[:, 9:12],
                          raw[:, 12], raw[:, 13], raw[:, 14], raw[:, 15], raw)


def _contact_metrics_of(raw: torch.Tensor) -> ContactMetrics:
    return ContactMetrics(*(raw[:, i] for i in range(CONTACT_PAIR)), raw)


def contact_readout_args(threshold=0.0, mode="abs", gain=1.0, span=(4.0, 4.0)):
    """``(threshold, mode, gain, (span_r, span_c))`` as floats, a mode name and a pair, checked against what
    ``tsr_contact_readout`` refuses; ``TactileSRHipError`` otherwise.  Host-only."""
    if not isinstance(mode, str) or mode not in CONTACT_MODES:
        raise TactileSRHipError(f"the contact threshold mode must be one of {sorted(CONTACT_MODES)}, got {mode!r}")
    try:
        thr, g = float(threshold), float(gain)
        sp = (float(span), float(span)) if isinstance(span, (int, float)) else tuple(float(s) for s in span)
    except (TypeError, ValueError) as e:
        raise TactileSRHipError(f"contact readout: {e}") from None
    if not _math.isfinite(thr):
        raise TactileSRHipError(f"the contact threshold must be finite, got {thr}")
    if mode == "range" and not 0.0 <= thr < 1.0:
        raise TactileSRHipError(f"a \"range\" contact threshold is a fraction in [0, 1), got {thr}")
    if not _math.isfinite(g):
        raise TactileSRHipError(f"the contact gain must be finite, got {g}")
    if len(sp) != 2 or not all(_math.isfinite(s) and s > 0 for s in sp):
        raise TactileSRHipError(f"the contact span is one or two positive finite numbers, got {span!r}")
    return thr, mode, g, sp


def _contact_image(y: torch.Tensor, who: str) -> torch.Tensor:
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise TactileSRHipError(f"{who} needs ROCm tensors (no CPU fallback)")
    if y.dtype != torch.float32:
        raise TactileSRHipError(f"{who} needs fp32 images, got {y.dtype}")
    if y.dim() == 3:
        y = y.unsqueeze(1)
    if y.dim() != 4 or y.shape[1] != 1 or y.shape[0] < 1 or not 1 <= y.shape[2] * y.shape[3] <= CONTACT_MAX_PIXELS:
        raise TactileSRHipError(f"{who} needs (B,1,H,W) or (B,H,W) images with B >= 1 and 1 <= H W <= 2^24, got "
                                f"{tuple(y.shape)}")
    return y.detach().contiguous()


def _contact_launch(y, t, args, rec_y, rec_t, pair, max_wgs=None):
    thr, mode, gain, span = args
    B, _, H, W = y.shape
    a = [ptr(y), ptr(t), _I(B), _I(H), _I(W), _I(CONTACT_MODES[mode]), _D(thr), _D(gain), _D(span[0]), _D(span[1]),
         ptr(rec_y), ptr(rec_t), ptr(pair)]
    if max_wgs is None:
        call("tsr_contact_readout", *a, stream())
    else:
        call("tsr_contact_readout_wgs", *a, _I(int(max_wgs)), stream())


def contact_readout(y: torch.Tensor, threshold: float = 0.0, mode: str = "abs", gain: float = 1.0, span=(4.0, 4.0),
                    max_wgs=None) -> ContactReadout:
    """The contact of every image of ``y`` ((B,1,H,W) or (B,H,W), fp32, on the device) from one
    ``tsr_contact_readout`` launch, no autograd: the pixels above the threshold -- ``mode="abs"``: ``v > threshold``;
    ``mode="range"``: ``v > mn + threshold (mx - mn)`` of the image's own range, at 0.5 the reference's binarisation
    (utility/raw_data_process.py:105-106) -- their count, area, mass (``gain`` times the masked sum), the image's total
    and peak, the peak position, the intensity-weighted centroid, central second moments, orientation and axes.
    ``span`` is the extent of the image in taxel pitches (rows, columns).  An image without contact has NaN geometry
    (centroid, moments, angle, axes); an image with a NaN or Inf has an all-NaN record.  Nothing is read back."""
    args = contact_readout_args(threshold, mode, gain, span)
    y = _contact_image(y, "contact_readout")
    if max_wgs is not None and int(max_wgs) < 1:
        raise TactileSRHipError(f"contact_readout: max_wgs must be at least 1, got {max_wgs}")
    raw = torch.empty(y.shape[0], CONTACT_REC, dtype=torch.float32, device=y.device)
    _contact_launch(y, None, args, raw, None, None, max_wgs)
    return _contact_readout_of(raw)


def contact_metrics(y: torch.Tensor, t: torch.Tensor, threshold: float = 0.0, mode: str = "abs", gain: float = 1.0,
                    span=(4.0, 4.0)):
    """``(ContactMetrics, readout_y, readout_t)`` of an output ``y`` and a target ``t`` of the same shape from one
    ``tsr_contact_readout`` launch: mask intersection, union, IoU and Dice, the centroid distance (pitch units), the
    relative mass error ``|M_y - M_t| / M_t``, the peak distance and the orientation difference folded into [0, pi/2],
    plus both images' own readouts.  Each image is thresholded against its own ``tau`` (``mode="range"``).  A value that
    needs a contact that is not there is NaN.  No resampling: a target on another grid goes through ``prepare_target``."""
    args = contact_readout_args(threshold, mode, gain, span)
    y = _contact_image(y, "contact_metrics")
    t = _contact_image(t, "contact_metrics")
    if t.shape != y.shape or t.device != y.device:
        raise TactileSRHipError(f"contact_metrics: the pair must share a shape and a device, got {tuple(y.shape)} on "
                                f"{y.device} and {tuple(t.shape)} on {t.device}")
    B = y.shape[0]
    rec = torch.empty(2, B, CONTACT_REC, dtype=torch.float32, device=y.device)
    pair = torch.empty(B, CONTACT_PAIR, dtype=torch.float32, device=y.device)
    _contact_launch(y, t, args, rec[0], rec[1], pair)
    return _contact_metrics_of(pair), _contact_readout_of(rec[0]), _contact_readout_of(rec[1])


@torch.no_grad()
def sr_readout(model, LR: torch.Tensor, **readout_kwargs):
    """``(out, readout)``: the model's eval forward on ``LR`` and the ``contact_readout`` of its output, under
    ``no_grad`` (the model's training flag is restored) -- the call a sensor loop makes.  ``readout_kwargs`` are those
    of ``contact_readout`` and are checked before the forward runs."""
    contact_readout_args(**{k: v for k, v in readout_kwargs.items() if k != "max_wgs"})
    if not model.training:                                          # the sensor loop: no walk over the modules
        out = model(LR)
    else:
        model.eval()
        try:
            out = model(LR)
        finally:
            model.train(True)
    return out, contact_readout(out.float(), **readout_kwargs)
