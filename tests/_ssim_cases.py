"""Shared by tests/test_ssim_cpu.py and tests/test_gpu_ssim.py: the yardstick of tsr_ssim_fwd_bwd
(include/tactilesr_hip.h), its inputs, its case tables and the rule the kernel is held to.

Yardstick: an fp64 torch restatement of the header's formulas -- the five moments as ``F.conv2d`` with the outer-product
Gaussian window (valid correlation), or as global means for ``win = 0`` -- and torch autograd for the gradient.  The same
code in fp32 is the "fp32 restatement": what a user composes from torch ops today.

Rule (the one tests/_tpsf_autograd.py uses), per image:

    max |kernel - fp64|  <=  max(1e-5 * scale, 4 * max |fp32 restatement - fp64|)

scale = 1 for values; for gradients the image's own max |d ssim / d y| in fp64 (zero-gradient images -- both zero, or
identical -- take the scale of the "clamped" law at the same shape and image index).  The second term allows a kernel
what plain fp32 arithmetic on the same inputs loses, and no more than four times that; it is capped:
tests/test_ssim_cpu.py asserts it is at most 1e-3 of the scale on every case below, so it cannot hide a failure.  The
tests print whether it was ever needed.

Inputs: targets are sums of three Gaussian blobs of amplitude <= 10 (a tactile contact image: mostly background).
Laws of the prediction:
  clamped    blobs + 0.5 N(0,1), clamped at 0            (a ReLU-like network output: the training state)
  signed     blobs + 0.5 N(0,1)                          (negative pixels: the products keep their sign)
  pedestal   both on a pedestal of 10, data_range 20     (the moments cancel hardest: E[x^2] ~ 100, variance ~ 0.25)
  dead       prediction == 0 against blobs               (the dead-network state: mx = sxx = sxt = 0)
  zeros      both == 0                                   (S == 1 everywhere, gradient exactly 0)
  identical  prediction == target                        (S == 1, gradient 0 up to rounding)
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

LAWS = ("clamped", "signed", "pedestal", "dead", "zeros", "identical")
K1, K2 = 0.01, 0.03
BAR = 1e-5
CAP = 1e-3           # the most the rule's second term may reach, as a fraction of the scale (asserted on the CPU)

# (name, B, H, W, win, sigma) and why the shape is there
WINDOW_CASES = [
    ("w11_1x11x11", 1, 11, 11, 11, 1.5),      # a single window position: the map is 1x1
    ("w11_3x11x12", 3, 11, 12, 11, 1.5),      # one map row, two columns
    ("w11_3x12x11", 3, 12, 11, 11, 1.5),      # two map rows, one column
    ("w11_3x13x29", 3, 13, 29, 11, 1.5),      # odd sizes, fewer rows than one step
    ("w11_2x21x21", 2, 21, 21, 11, 1.5),      # more dy rows than one 16-row step; the second step has no new map row
    ("w11_5x40x40", 5, 40, 40, 11, 1.5),      # the training shape: three steps, the ring wraps
    ("w11_2x100x100", 2, 100, 100, 11, 1.5),  # tPSFNet's HR shape: a step shorter than 16 rows, the large LDS budget
    ("w11_2x124x124", 2, 124, 124, 11, 1.5),  # the training limit (scale_factor 31)
    ("w11_1x128x128", 1, 128, 128, 11, 1.5),  # the largest supported image
    ("w11_2x128x11", 2, 128, 11, 11, 1.5),    # tall and one map column wide
    ("w7_3x13x29", 3, 13, 29, 7, 1.0),        # another window instantiation
    ("w7_2x40x40", 2, 40, 40, 7, 1.0),
    ("w3_1x3x3", 1, 3, 3, 3, 0.5),            # the smallest window on the smallest image
    ("w3_2x5x7", 2, 5, 7, 3, 0.5),
]
GLOBAL_CASES = [
    ("g_3x1x7", 3, 1, 7, 0, 0.0),             # fewer pixels than threads
    ("g_1x1x1", 1, 1, 1, 0, 0.0),             # one pixel: every variance is exactly 0
    ("g_4x40x40", 4, 40, 40, 0, 0.0),         # eval_func's shape
    ("g_2x100x100", 2, 100, 100, 0, 0.0),
]
CASES = {c[0]: c for c in WINDOW_CASES + GLOBAL_CASES}


def constants(data_range):
    return (K1 * data_range) ** 2, (K2 * data_range) ** 2


def gauss(win, sigma):
    k = torch.arange(win, dtype=torch.float64) - (win - 1) / 2
    g = torch.exp(-k * k / (2 * sigma * sigma))
    return g / g.sum()


def restatement(y, t, win, sigma, C1, C2):
    """Per-image SSIM (B,) of (B,1,H,W) tensors in their own dtype; differentiable."""
    if win == 0:
        def G(z):
            return z.mean(dim=(1, 2, 3), keepdim=True)
    else:
        g = gauss(win, sigma)
        w = torch.outer(g, g).to(y.dtype).to(y.device)[None, None]

        def G(z):
            return F.conv2d(z, w)
    mx, mt = G(y), G(t)
    sxx, stt, sxt = G(y * y) - mx * mx, G(t * t) - mt * mt, G(y * t) - mx * mt
    S = ((2 * mx * mt + C1) * (2 * sxt + C2)) / ((mx * mx + mt * mt + C1) * (sxx + stt + C2))
    return S.mean(dim=(1, 2, 3))


def values_and_grads(y, t, win, sigma, C1, C2, dtype):
    """(ssim (B,), d ssim_b / d y (B,1,H,W)) of the restatement in `dtype`."""
    yy = y.detach().to(dtype).clone().requires_grad_(True)
    v = restatement(yy, t.detach().to(dtype), win, sigma, C1, C2)
    v.sum().backward()                   # images are independent: row b of the gradient is d ssim_b / d y_b
    return v.detach(), yy.grad.detach()


def closed_form(y, t, win, sigma, C1, C2):
    """The header's P / Q / R form of the gradient in fp64 (B,1,H,W)."""
    y, t = y.double(), t.double()
    if win == 0:
        n = y.shape[2] * y.shape[3]

        def G(z):
            return z.mean(dim=(1, 2, 3), keepdim=True)

        def GT(z):
            return (z / n).expand_as(y)
    else:
        g = gauss(win, sigma)
        w = torch.outer(g, g)[None, None]

        def G(z):
            return F.conv2d(z, w)

        def GT(z):
            return F.conv_transpose2d(z, w)
    mx, mt = G(y), G(t)
    sxx, stt, sxt = G(y * y) - mx * mx, G(t * t) - mt * mt, G(y * t) - mx * mt
    A1, A2, B1, B2 = 2 * mx * mt + C1, 2 * sxt + C2, mx * mx + mt * mt + C1, sxx + stt + C2
    S = A1 * A2 / (B1 * B2)
    P = 2 * mt * (A2 - A1) / (B1 * B2) - 2 * mx * S * (1 / B1 - 1 / B2)
    Q = -S / B2
    R = 2 * A1 / (B1 * B2)
    N = S.shape[2] * S.shape[3]
    return (GT(P) + 2 * y * GT(Q) + t * GT(R)) / N


def brute_force(y, t, win, sigma, C1, C2):
    """SSIM of ONE (H,W) pair with python floats and explicit loops over map positions and taps."""
    H, W = y.shape
    y, t = y.tolist(), t.tolist()
    g = gauss(win, sigma).tolist() if win else None
    positions = [(0, 0)] if win == 0 else [(m, j) for m in range(H - win + 1) for j in range(W - win + 1)]
    total = 0.0
    for m, j in positions:
        taps = ([(r, c, 1.0 / (H * W)) for r in range(H) for c in range(W)] if win == 0 else
                [(m + a, j + b, g[a] * g[b]) for a in range(win) for b in range(win)])
        mx = math.fsum(wt * y[r][c] for r, c, wt in taps)
        mt = math.fsum(wt * t[r][c] for r, c, wt in taps)
        sxx = math.fsum(wt * y[r][c] * y[r][c] for r, c, wt in taps) - mx * mx
        stt = math.fsum(wt * t[r][c] * t[r][c] for r, c, wt in taps) - mt * mt
        sxt = math.fsum(wt * y[r][c] * t[r][c] for r, c, wt in taps) - mx * mt
        total += ((2 * mx * mt + C1) * (2 * sxt + C2)) / ((mx * mx + mt * mt + C1) * (sxx + stt + C2))
    return total / len(positions)


def blobs(B, H, W, gen):
    """(B,1,H,W) fp32: three Gaussian blobs per image, amplitudes in (2, 10), centres anywhere, widths from the image size."""
    r = torch.arange(H, dtype=torch.float32)[None, :, None]
    c = torch.arange(W, dtype=torch.float32)[None, None, :]
    img = torch.zeros(B, H, W)
    for _ in range(3):
        amp = 2 + 8 * torch.rand(B, 1, 1, generator=gen)
        cr = torch.rand(B, 1, 1, generator=gen) * H
        cc = torch.rand(B, 1, 1, generator=gen) * W
        s = (0.04 + 0.08 * torch.rand(B, 1, 1, generator=gen)) * max(H, W, 8)    # contacts are small: mostly background
        img = img + amp * torch.exp(-((r - cr) ** 2 + (c - cc) ** 2) / (2 * s * s))
    return (img * (10.0 / img.amax(dim=(1, 2), keepdim=True).clamp_min(10.0)))[:, None].contiguous()


def make_pair(B, H, W, law, seed):
    """(prediction, target, data_range), fp32 CPU."""
    gen = torch.Generator().manual_seed(seed)
    t = blobs(B, H, W, gen)
    if H * W == 1:
        # A single pixel has no variance: S = (2xt + C1) / (x^2 + t^2 + C1) exactly, and the variance terms of the
        # gradient cancel to 0 at a ratio of x^2 / C2.  At amplitude 10 that is 1e5 and the fp32 restatement is off
        # by 1.4e-2 of the scale, far past the cap on the rule's second term; at amplitude 0.1 the ratio is 11.
        t = t * 0.01
    noisy = t + 0.5 * torch.randn(B, 1, H, W, generator=gen)
    if law == "clamped":
        return noisy.clamp_min(0).contiguous(), t, 1.0
    if law == "signed":
        return noisy, t, 1.0
    if law == "pedestal":
        return noisy + 10.0, t + 10.0, 20.0
    if law == "dead":
        return torch.zeros_like(t), t, 1.0
    if law == "zeros":
        return torch.zeros_like(t), torch.zeros_like(t), 1.0
    if law == "identical":
        return t.clone(), t, 1.0
    raise KeyError(law)


@functools.lru_cache(maxsize=None)
def reference(name, law):
    """Everything a test needs of one (case, law), computed once and never modified:
    dict(y, t, data_range, C1, C2, win, sigma, v64, g64, v32, g32, scale (B,) gradient scale per image)."""
    _, B, H, W, win, sigma = CASES[name]
    y, t, data_range = make_pair(B, H, W, law, zlib.crc32(name.encode()))
    scale = reference(name, "clamped")["scale"] if law in ("zeros", "identical") else None
    return build_reference(y, t, win, sigma, data_range, scale)


def build_reference(y, t, win, sigma, data_range=1.0, scale=None):
    """The reference dict of any fp32 CPU pair; `scale` (B,) overrides the images' own gradient scale."""
    C1, C2 = constants(data_range)
    v64, g64 = values_and_grads(y, t, win, sigma, C1, C2, torch.float64)
    v32, g32 = values_and_grads(y, t, win, sigma, C1, C2, torch.float32)
    if scale is None:
        scale = g64.abs().amax(dim=(1, 2, 3))
    return dict(y=y, t=t, data_range=data_range, C1=C1, C2=C2, win=win, sigma=sigma, v64=v64, g64=g64, v32=v32, g32=g32,
                scale=scale)


IMPULSE_SHAPES = [(13, 29), (40, 40)]


def impulse_positions(H, W, win):
    """Corners, edge midpoints, the first pixel every window row / column reaches, and the centre."""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1),
            (win - 1, win - 1), (H // 2, W // 2)]


@functools.lru_cache(maxsize=None)
def impulse_reference(H, W, win=11, sigma=1.5):
    """One image per position p: prediction = target + e_p on one blob target.  The gradient is the adjoint's response
    to a single pixel: a wrong halo row or a shifted adjoint index moves it as a whole.  The scale is each image's own
    max |gradient|, which a corner impulse makes tiny (its weight is g[0]^2): the fp32 restatement is off by up to a
    quarter of that scale there, so on these images the rule's second term is only ever the cap `check` clamps it to
    (1e-3 of the scale), not the four-fold fp32 error the CPU test caps on every other table."""
    pos = impulse_positions(H, W, win)
    _, t, _ = make_pair(1, H, W, "identical", 7000 + H * 131 + W)
    t = t.expand(len(pos), 1, H, W).contiguous()
    y = t.clone()
    for b, (r, c) in enumerate(pos):
        y[b, 0, r, c] += 1.0
    return build_reference(y, t, win, sigma)


WALK = (2100, 11, 13)


@functools.lru_cache(maxsize=None)
def walk_reference():
    """2100 distinct 11x13 images (a 1x3 map each): more images than any grid cap the launch could have."""
    B, H, W = WALK
    y, t, dr = make_pair(B, H, W, "clamped", 2100)
    return build_reference(y, t, 11, 1.5, dr)


def second_term(ref):
    """The rule's second term as fractions of the scale, per image: (values (B,), gradients (B,))."""
    fv = 4 * (ref["v32"].double() - ref["v64"]).abs()
    eg, scale = 4 * (ref["g32"].double() - ref["g64"]).abs().amax(dim=(1, 2, 3)), ref["scale"]
    fg = torch.where(scale > 0, eg / scale, torch.where(eg == 0, torch.zeros_like(eg), torch.full_like(eg, math.inf)))
    return fv, fg


class Worst:
    """Worst fractions seen over a table: the kernel's error and the fp32 restatement's, in units of the scale."""

    def __init__(self):
        self.kernel_v = self.kernel_g = self.fp32_v = self.fp32_g = 0.0
        self.second_term_needed = False

    def line(self, label):
        return (f"[ssim] {label}: kernel value {self.kernel_v:.2e} gradient {self.kernel_g:.2e} | fp32 restatement value "
                f"{self.fp32_v:.2e} gradient {self.fp32_g:.2e} | second term needed: {self.second_term_needed}")


def check(ref, vals, grad, worst=None, grad_factor=1.0, prior=None, label=""):
    """Hold kernel output (`vals` (B,) fp32, `grad` (B,1,H,W) fp32 or None; CPU tensors) to the rule.  With
    `grad_factor` / `prior` the gradient is expected as prior + grad_factor * d ssim / d y (the dy contract); the scale
    is |grad_factor| times the image's, so a prior should be of that size for the bar to mean what it says."""
    fv, fg = second_term(ref)
    ev = (vals.double() - ref["v64"]).abs()
    assert not torch.isnan(ev).any(), (label, "NaN value")
    bar_v = torch.maximum(torch.full_like(fv, BAR), fv.clamp_max(CAP))
    if worst is not None:
        worst.kernel_v = max(worst.kernel_v, float(ev.max()))
        worst.fp32_v = max(worst.fp32_v, float(fv.max()) / 4)
        worst.second_term_needed |= bool((ev > BAR).any())
    assert (ev <= bar_v).all(), (label, "value", ev.tolist(), bar_v.tolist())
    if grad is None:
        return
    want = grad_factor * ref["g64"]
    if prior is not None:
        want = want + prior.double()
    eg = (grad.double() - want).abs().amax(dim=(1, 2, 3))
    assert not torch.isnan(eg).any(), (label, "NaN gradient")
    if grad_factor == 0:
        assert torch.equal(grad, prior if prior is not None else torch.zeros_like(grad)), (label, "dy_scale 0")
        return
    scale = ref["scale"] * abs(grad_factor)
    frac = torch.where(scale > 0, eg / scale, torch.where(eg == 0, torch.zeros_like(eg), torch.full_like(eg, math.inf)))
    bar_g = torch.maximum(torch.full_like(fg, BAR), fg.clamp_max(CAP))      # never past the cap (the impulse images)
    if worst is not None:
        worst.kernel_g = max(worst.kernel_g, float(frac.max()))
        worst.fp32_g = max(worst.fp32_g, float(fg.max()) / 4)
        worst.second_term_needed |= bool((frac > BAR).any())
    assert (frac <= bar_g).all(), (label, "gradient", frac.tolist(), bar_g.tolist())


BASE_ARGS = dict(y=1, t=1, B=2, H=13, W=29, win=11, sigma=1.5, C1=1e-4, C2=9e-4, ssim=1, dy=1, dy_scale=1.0, accumulate=0)
NAN = float("nan")
# every refusal include/tactilesr_hip.h lists: (label, overrides of BASE_ARGS); pointers: 1 = given, 0 = NULL
REFUSALS = [
    ("null y", dict(y=0)), ("null t", dict(t=0)), ("null ssim", dict(ssim=0)),
    ("B 0", dict(B=0)), ("B -1", dict(B=-1)), ("H 0", dict(H=0)), ("W 0", dict(W=0)), ("H -3", dict(H=-3)),
    ("W -3", dict(W=-3)), ("global H 0", dict(win=0, H=0)),
    ("win -1", dict(win=-1)), ("win -11", dict(win=-11)), ("win 1", dict(win=1)), ("win 2", dict(win=2)),
    ("win 4", dict(win=4)), ("win 10", dict(win=10)), ("win 12", dict(win=12)), ("win 13", dict(win=13)),
    ("H below win", dict(H=10)), ("W below win", dict(W=10)), ("H 129", dict(H=129)), ("W 129", dict(W=129)),
    ("sigma 0", dict(sigma=0.0)), ("sigma -1", dict(sigma=-1.0)), ("sigma NaN", dict(sigma=NAN)),
    ("C1 0", dict(C1=0.0)), ("C1 -1", dict(C1=-1.0)), ("C1 NaN", dict(C1=NAN)),
    ("C2 0", dict(C2=0.0)), ("C2 -1", dict(C2=-1.0)), ("C2 NaN", dict(C2=NAN)),
    ("global C1 NaN", dict(win=0, C1=NAN)),
    ("accumulate 2", dict(accumulate=2)), ("accumulate -1", dict(accumulate=-1)),
    ("dy_scale NaN", dict(dy_scale=NAN)), ("dy_scale NaN, no dy", dict(dy_scale=NAN, dy=0)),
    ("global above 2^28", dict(win=0, H=1 << 15, W=(1 << 13) + 1)),
]


def call_raw(lib, a, y=0, t=0, ssim=0, dy=0, stream=0):
    """tsr_ssim_fwd_bwd with the scalars of `a` and the given addresses; returns the status."""
    import ctypes
    P = ctypes.c_void_p
    return lib.tsr_ssim_fwd_bwd(P(y), P(t), a["B"], a["H"], a["W"], a["win"], ctypes.c_double(a["sigma"]),
                                ctypes.c_double(a["C1"]), ctypes.c_double(a["C2"]), P(ssim), P(dy),
                                ctypes.c_float(a["dy_scale"]), a["accumulate"], P(stream))
