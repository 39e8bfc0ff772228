"""Comparator and CPU references of the weight-gradient kernel tests (test_gpu_wgrad.py; self-test: test_wgrad_check_cpu.py).

A weight gradient dW[C_out][C_in][k][k] is compared with an fp64 reference in two ways:

  * GLOBAL: max|dW - ref| / max|ref| < 1e-5, the project's bar for every train arithmetic (test_gpu_train.py); the same for
    the bias gradient db;
  * SLICE-WISE: the same relative max-norm inside every [64 C_out][64 C_in][kh][kw] slice, each against its OWN maximum.  A
    wrong tap, a wrong kernel-row group or a wrong 64-channel block is one slice, and an error that exists only where an image
    edge cuts a patch is no longer diluted by a large neighbouring block.  The bar of a slice is max(1e-5, 4 * e_ref): e_ref is
    the slice-wise error of torch's own fp32 CPU autograd against the same fp64 reference on the same operands (how far fp32
    summation alone moves that slice), the factor 4 allows for another summation order.  A slice whose reference is
    identically zero (taps that never meet an in-image pixel pair, e.g. the outer taps of a 1x1 image) must be exactly zero.

Everything here is plain CPU torch: no library call, no device.
"""
import numpy as np
import torch
import torch.nn.functional as F

GLOBAL_BAR = 1e-5
SLICE_FLOOR = 1e-5
SLICE_FACTOR = 4.0


def q16(t):
    """Round to bf16 (nearest even) and back to fp32."""
    return t.bfloat16().float()


def fma32(x, s, t):
    """fp32 fma(x, s_c, t_c) per channel, as the kernels form a virtual input: the product is exact in fp64."""
    return (x.double() * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)).float()


def conv_wgrad(a, dz, ks):
    """dW of conv2d(a, W, stride 1, pad ks // 2) given the output gradient dz, by torch autograd in the dtype of `a`."""
    w = torch.zeros(dz.shape[1], a.shape[1], ks, ks, dtype=a.dtype, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(a, w, padding=ks // 2), w, dz.to(a.dtype))
    return gw


def _slices(t):
    co, ci, kh, kw = t.shape
    assert co % 64 == 0 and ci % 64 == 0
    return t.reshape(co // 64, 64, ci // 64, 64, kh, kw)


def slice_errors(got, ref):
    """Per [64 C_out][64 C_in][kh][kw] slice: max|got - ref| / max|ref| of that slice, shape [C_out/64][C_in/64][k][k].
    A slice whose reference is all zero gives 0 if `got` is exactly zero there and inf otherwise."""
    d = _slices((got.double() - ref.double()).abs()).amax(dim=(1, 3))
    m = _slices(ref.double().abs()).amax(dim=(1, 3))
    rel = d / m.clamp_min(1e-300)
    zero = m == 0
    rel[zero] = torch.where(d[zero] == 0, torch.zeros_like(d[zero]), torch.full_like(d[zero], float("inf")))
    return rel


def global_error(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def reference(a, dz, ks):
    """fp64 reference of one case and the yardstick of its slice bars.  a, dz: the fp32 operand values the matrix cores see
    (already rounded for the bf16 arithmetics).  Returns {"dw": fp64 dW, "e_ref": slice-wise error of torch's fp32 CPU
    autograd on the same operands}."""
    dw = conv_wgrad(a.double(), dz.double(), ks)
    e_ref = slice_errors(conv_wgrad(a.float(), dz.float(), ks), dw)
    return {"dw": dw, "e_ref": e_ref}


def check_dw(got, ref, label=""):
    """Both bars on a weight gradient (`got`: fp32 [C_out][C_in][k][k] on the CPU; `ref`: what reference() returned).
    Returns (global error, worst slice error / its bar, text); raises AssertionError naming the worst slice."""
    assert got.shape == ref["dw"].shape, (got.shape, ref["dw"].shape)
    assert torch.isfinite(got).all(), f"{label}: non-finite dW"
    e = global_error(got, ref["dw"])
    rel = slice_errors(got, ref["dw"])
    bar = torch.clamp(SLICE_FACTOR * ref["e_ref"], min=SLICE_FLOOR)
    ratio = rel / bar
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    r = float(ratio.reshape(-1)[worst])
    txt = (f"{label}: dW global {e:.2e}; worst slice (co block {idx[0]}, ci block {idx[1]}, tap {idx[2]},{idx[3]}) "
           f"error {float(rel[idx]):.2e} = {r:.3f} of its bar {float(bar[idx]):.2e} (e_ref {float(ref['e_ref'][idx]):.2e})")
    print(txt)
    assert e < GLOBAL_BAR, txt
    assert r < 1.0, txt
    return e, r, txt


def check_db(got, ref_db, label=""):
    """The global bar on a bias gradient (fp64 reference: sum of dz over batch and pixels)."""
    assert torch.isfinite(got).all(), f"{label}: non-finite db"
    e = global_error(got, ref_db)
    print(f"{label}: db {e:.2e}")
    assert e < GLOBAL_BAR, f"{label}: db {e:.2e}"
    return e
