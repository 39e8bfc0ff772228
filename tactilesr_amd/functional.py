"""HIP-backed functional pieces of the SR training / eval step that sit outside the model:
target preparation, MSE loss, PSNR / SSIM, the differentiable SSIM and the MSE + SSIM loss (reference
train/tactileSR_train.py:41-51,66-101; utility/tools.py:49-114), and the pixel losses with a contact weight
(L1 / Charbonnier / Huber: not in the reference, whose criterion is nn.MSELoss)."""
from __future__ import annotations

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


def _ssim_launch(y: torch.Tensor, t: torch.Tensor, data_range, window, sigma, K1, K2, dy, dy_scale, accumulate):
    """One ``tsr_ssim_fwd_bwd`` launch on contiguous fp32 (B,1,H,W) tensors: the per-sample values; ``dy`` (or None)
    is written / accumulated in place."""
    if y.dim() != 4 or y.shape[1] != 1 or t.shape != y.shape:
        raise TactileSRHipError(f"ssim needs two (B,1,H,W) tensors of one shape, got {tuple(y.shape)} and {tuple(t.shape)}")
    B, _, H, W = y.shape
    vals = torch.empty(B, dtype=torch.float32, device=y.device)
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


def _plain_mse(pixel_kind, fg_weight) -> bool:
    return str(pixel_kind).lower() == "mse" and float(fg_weight) == 0


def sr_loss_fwd_bwd(y: torch.Tensor, target: torch.Tensor, ssim_weight: float = 0.0, data_range: float = 1.0,
                    window: int = 11, sigma: float = 1.5, K1: float = 0.01, K2: float = 0.03, return_parts: bool = False,
                    pixel_kind: str = "mse", pixel_param=None, fg_weight: float = 0.0, fg_threshold: float = 0.0):
    """``pixel(y, target) + ssim_weight * (1 - mean_b ssim_b)`` and its gradient w.r.t. ``y``, outside autograd:
    ``(loss (1,), dy)``.  The pixel launch, then the SSIM launch accumulating ``-ssim_weight / B * d ssim_b / d y`` into
    the same ``dy``.  The pixel term is the MSE launch (``mse_fwd_bwd``) for ``pixel_kind="mse"`` with ``fg_weight == 0``,
    otherwise ``pixel_loss_fwd_bwd`` with the four pixel arguments; ``ssim_weight == 0`` is that launch alone, launch
    for launch.  ``return_parts=True`` appends the two terms: ``(loss, dy, pixel (1,), ssim (B,) or None)``."""
    if not y.is_cuda or not target.is_cuda:
        raise TactileSRHipError("sr_loss_fwd_bwd needs ROCm tensors (no CPU fallback)")
    if _plain_mse(pixel_kind, fg_weight):
        mse, dy = mse_fwd_bwd(y, target)
    else:
        mse, dy = pixel_loss_fwd_bwd(y, target, pixel_kind, pixel_param, fg_weight, fg_threshold)
    if ssim_weight == 0:
        return (mse, dy, mse, None) if return_parts else (mse, dy)
    t = target.detach().float().contiguous()
    vals = _ssim_launch(y.contiguous(), t, data_range, window, sigma, K1, K2, dy, -float(ssim_weight) / y.shape[0], 1)
    loss = mse + float(ssim_weight) * (1.0 - vals.mean())
    return (loss, dy, mse, vals) if return_parts else (loss, dy)


class _SRLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, target, ssim_weight, data_range, window, sigma, pixel_kind, pixel_param, fg_weight, fg_threshold):
        loss, dy, mse, vals = sr_loss_fwd_bwd(y, target, ssim_weight, data_range, window, sigma, return_parts=True,
                                              pixel_kind=pixel_kind, pixel_param=pixel_param, fg_weight=fg_weight,
                                              fg_threshold=fg_threshold)
        ctx.save_for_backward(dy)
        mse0 = mse[0]
        ctx.mark_non_differentiable(mse0, vals)
        return loss[0], mse0, vals

    @staticmethod
    def backward(ctx, gout, _gmse, _gvals):
        (dy,) = ctx.saved_tensors
        return (dy * gout,) + (None,) * 9


def sr_loss(y: torch.Tensor, target: torch.Tensor, ssim_weight: float, data_range: float = 1.0, window: int = 11,
            sigma: float = 1.5, pixel_kind: str = "mse", pixel_param=None, fg_weight: float = 0.0,
            fg_threshold: float = 0.0):
    """The autograd form of ``sr_loss_fwd_bwd`` for ``ssim_weight != 0``: ``(loss, pixel term, per-sample ssim)``; only
    ``loss`` carries a gradient (to ``y``)."""
    if not y.is_cuda:
        raise TactileSRHipError("sr_loss needs ROCm tensors (no CPU fallback)")
    return _SRLoss.apply(y.float(), target, float(ssim_weight), data_range, window, sigma, pixel_kind, pixel_param,
                         fg_weight, fg_threshold)


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
