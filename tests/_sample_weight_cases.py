"""Yardstick, case tables, checker and launch harness of the per-sample supervision-weight tests (tsr_sample_scale,
tsr_pixel_loss_ps_fwd_bwd[_wgs], tsr_ssim_fwd_bwd_ps, tsr_weighted_mean).  Nothing at import time touches a device:
tests/test_sample_weight_cpu.py checks every precondition the GPU tests rely on.

The yardstick is the operator of include/tactilesr_hip.h restated in torch ops (fp64; differentiable by autograd), for B
images of P pixels, omega_p = 1 + fg_weight [t_p > fg_threshold] and rho the pixel kind of tests/_pixel_loss_cases.py:

    valid(w) = w finite and >= 0,   D = sum of the valid w_b (fp64, index order)
    s_b = NaN where w_b is invalid, else  "sum": fl32(w_b B / D) (0 when D == 0),  "batch": w_b
    pix_b = (1/P) sum_p omega_p rho(d_p)
    L     = (1/B) sum_{s_b != 0} s_b [pix_b + ls (1 - ssim_b)]
    dL/dy_bp = (s_b/B) [omega_p rho'(d_p)/P - ls d ssim_b/d y_bp],   a sample with s_b == 0 contributes exact zeros

ssim_b and its gradient are those of tests/_ssim_cases.py.  A skipped sample (s_b == 0) is taken out BEFORE any arithmetic
(`masked`): its pixels may be NaN, and 0 x NaN must not reach the yardstick either.

THE RULE for every comparison:  |kernel - fp64| <= 1e-5 x scale, the scale being the quantity's own: the image's max |dy|
for a gradient, pix_b for a per-sample value, the loss for the loss.  The same restatement evaluated in fp32 stays below
FP32_BAR = 1e-6 of those scales on every case of the tables (asserted on the CPU), so the bar keeps a factor of 10 over
plain fp32 arithmetic.

Inputs are those of the pixel-loss tests (`_pixel_loss_cases.make_inputs`): sparse non-negative targets, predictions
relu(t + noise), exact ties and elements at |d| == delta, laid out over the (B, P) batch by flat index.
"""
import ctypes
import functools
import math

import torch

import _pixel_loss_cases as PC
import _ssim_cases as SC

BAR = 1e-5
FP32_BAR = 1e-6
NAN, INF = float("nan"), float("inf")
NORMS = {"sum": 0, "batch": 1}            # the mode codes of the ABI
MAX_WGS = 2048                            # TSR_PIXEL_LOSS_PS_MAX_WGS
THREADS = 256                             # a workgroup of the per-image launch: thread k owns quads k, k + 256, ...

# (H, W): why
SHAPES = {
    (1, 1): "one pixel: one thread has work, a ragged quad of one element",
    (5, 7): "odd sizes: 35 elements, the scalar path with a ragged last quad (3 of 4)",
    (3, 127): "P % 4 == 1: the scalar path over 96 quads, the last of one element",
    (40, 40): "the train step's output at scale factor 10: 400 quads, threads with one and with two",
    (100, 100): "the reference's own grid: 2500 quads, ten per thread and a ragged round",
    (128, 128): "the bound of the SSIM and degradation launches: 16 whole rounds of quads",
}
BATCHES = (1, 7, 67)                      # one image; a few; more than a small grid cap
# (kind, param): every kind of the pixel launch (both Charbonnier eps and both Huber deltas of its table)
KINDS = PC.KINDS
# (fg_weight, fg_threshold): no contact weight, and 4 on the pixels above 0.5
CONTACT = [(0.0, 0.0), (4.0, 0.5)]
PARAMS = [(k, p, w, th) for k, p in KINDS for w, th in CONTACT]
WALK = (2100, 5, 7)                       # more distinct images than the default grid cap
INVALID_B = 600                           # invalid weights among 600 samples: three chunks of the one-workgroup sum's staging


# ------------------------------------------------------------------------------------------------------------ the yardstick
def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def valid(w):
    return torch.isfinite(w) & (w >= 0)


def scale_ref(w, norm):
    """(s (B,) fp32, D as a python float, the number of valid weights > 0) of an fp32 CPU weight vector: D summed in fp64
    in index order, s_b = fl32(w_b B / D) evaluated in fp64 and rounded once."""
    assert w.dtype == torch.float32 and w.dim() == 1 and norm in NORMS
    B, ok = w.shape[0], valid(w)
    D = 0.0
    for v, k in zip(w.tolist(), ok.tolist()):
        if k:
            D += v                                                    # python floats are fp64; index order
    if norm == "batch":
        s = w.clone()
    elif D == 0:
        s = torch.zeros(B)
    else:
        s = ((w.double() * float(B)) / D).float()
    s = torch.where(ok, s, torch.full((B,), NAN))
    return s, D, int((ok & (w > 0)).sum())


def kept(s):
    """The samples that are not skipped: s_b != 0 (a NaN scale is kept, and poisons its sample)."""
    return s != 0


def masked(x, s):
    """x (B, ...) with the skipped samples replaced by zeros (never multiplied: they may hold NaN)."""
    k = kept(s).view(-1, *([1] * (x.dim() - 1)))
    return torch.where(k, x, torch.zeros_like(x))


def rho(d, kind, param):
    if kind == "mse":
        return d * d
    if kind == "l1":
        return d.abs()
    if kind == "charbonnier":
        return torch.sqrt(d * d + param * param)
    if kind == "huber":
        a = d.abs()
        return torch.where(a <= param, 0.5 * d * d, param * (a - 0.5 * param))
    raise ValueError(kind)


def per_sample(y, t, kind, param=None, fg_weight=0.0, fg_threshold=0.0):
    """pix (B,) in y's dtype from plain torch ops; y, t (B, ...)."""
    B = y.shape[0]
    yy, tt = y.reshape(B, -1), t.reshape(B, -1)
    return (PC.weights(tt, fg_weight, fg_threshold, y.dtype) * rho(yy - tt, kind, param)).sum(dim=1) / yy.shape[1]


def restatement(y, t, s, kind, param=None, fg_weight=0.0, fg_threshold=0.0, ssim_weight=0.0, ssim_args=None):
    """(L, pix (B,)) in y's dtype: the weighted loss of the module docstring (differentiable in y) and the per-sample
    pixel values, zeros for the skipped.  `ssim_args` = (win, sigma, C1, C2) for a non-zero `ssim_weight`: y, t are then
    (B,1,H,W)."""
    B = y.shape[0]
    sd = masked(s.to(y.dtype), s)
    ym, tm = masked(y, s), masked(t, s)
    pix = masked(per_sample(ym, tm, kind, param, fg_weight, fg_threshold), s)
    term = pix
    if ssim_weight:
        term = term + ssim_weight * (1 - SC.restatement(ym, tm, *ssim_args))
    return (sd * masked(term, s)).sum() / B, pix


def closed_form(y, t, s, kind, param=None, fg_weight=0.0, fg_threshold=0.0):
    """(pix (B,), dL/dy of y's shape) of the pixel term in fp64 without autograd: (s_b/B) omega rho'(d) / P with
    sign(0) = 0, exact zeros for the skipped."""
    B = y.shape[0]
    ym, tm = masked(y.double(), s), masked(t.double(), s)
    P = ym.numel() // B
    g = PC.closed_form(ym, tm, kind, param, fg_weight, fg_threshold) * ym.numel() / P      # omega rho'(d) / P
    sd = masked(s.double(), s).view(-1, *([1] * (y.dim() - 1)))
    return masked(per_sample(ym, tm, kind, param, fg_weight, fg_threshold), s), masked(sd * g / B, s)


def autograd_grads(y, t, s, kind, param, fg_weight, fg_threshold, dtype):
    """(L, pix, dL/dy) of the restatement through autograd in `dtype`."""
    yy = y.detach().to(dtype).clone().requires_grad_(True)
    L, pix = restatement(yy, t.detach().to(dtype), s, kind, param, fg_weight, fg_threshold)
    (g,) = torch.autograd.grad(L, yy, allow_unused=True)
    return L.detach(), pix.detach(), (g if g is not None else torch.zeros_like(yy))


# ------------------------------------------------------------------------------------------------------------------- inputs
def weights_for(B, pattern, seed=0):
    """(B,) fp32 weights.  "ones"; "binary": 1, 0, 1, 0, ... (the first sample labeled); "zeros"; "fractional": uniform in
    (0, 2) with every fifth sample 0 and one 0.5 / one 1 exactly; "invalid": "fractional" with a negative, a NaN, a +Inf
    and a -Inf weight spread over the batch."""
    g = torch.Generator().manual_seed(900 + seed)
    if pattern == "ones":
        return torch.ones(B)
    if pattern == "zeros":
        return torch.zeros(B)
    if pattern == "binary":
        return (torch.arange(B) % 2 == 0).float()
    w = 2 * torch.rand(B, generator=g) + 1e-3
    w[torch.arange(B) % 5 == 4] = 0.0
    w[0] = 0.5
    if B > 1:
        w[1] = 1.0
    if pattern == "invalid":
        for frac, bad in ((0.1, -1.0), (0.45, NAN), (0.8, INF), (0.95, -INF)):
            w[int(frac * (B - 1))] = bad
    else:
        assert pattern == "fractional", pattern
    return w


@functools.lru_cache(maxsize=None)
def inputs(H, W, B):
    """(y, t) fp32 of shape (B, H*W), computed once; treat as read-only."""
    return PC.make_inputs((B, H * W), 5000 + 100 * H + 10 * W + B)


def poisoned(y, t, s):
    """Copies of y, t with NaN / Inf filling the skipped samples (alternating per sample)."""
    y, t = y.clone(), t.clone()
    for n, b in enumerate(torch.nonzero(~kept(s)).flatten().tolist()):
        y[b], t[b] = (NAN, INF) if n % 2 == 0 else (-INF, NAN)
    return y, t


def build_reference(y, t, s, kind, param, fg_weight, fg_threshold):
    pix, dy = closed_form(y, t, s, kind, param, fg_weight, fg_threshold)
    L32, pix32, dy32 = autograd_grads(y, t, s, kind, param, fg_weight, fg_threshold, torch.float32)
    L64 = float((masked(s.double(), s) * pix).sum() / y.shape[0])
    return dict(y=y, t=t, s=s, kind=kind, param=param, fg_weight=fg_weight, fg_threshold=fg_threshold, pix=pix, dy=dy, L=L64,
                L32=float(L32), pix32=pix32, dy32=dy32)


@functools.lru_cache(maxsize=64)
def reference(H, W, B, pattern, norm, kind, param, fg_weight, fg_threshold):
    """Computed once per case and shared; treat as read-only."""
    y, t = inputs(H, W, B)
    s = scale_ref(weights_for(B, pattern, seed=B), norm)[0]
    return build_reference(y, t, s, kind, param, fg_weight, fg_threshold)


# ------------------------------------------------------------------------------------------------------------------ checker
def frac(err, scale):
    """Per-sample err / scale with 0 / 0 = 0; the worst."""
    out = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err),
                                                                            torch.full_like(err, math.inf)))
    return float(out.max())


def fractions(ref, pix=None, dy=None, dt=None, dy_scale=1.0, prior=None, L=None):
    """Worst per-sample fraction of the scale for each given output (fp32 CPU tensors), as a dict."""
    B = ref["y"].shape[0]
    c = f32(dy_scale)
    out = {}
    if pix is not None:
        out["pix"] = frac((pix.double() - ref["pix"]).abs(), ref["pix"].abs())
    scale = abs(c) * ref["dy"].reshape(B, -1).abs().amax(dim=1)
    if dy is not None:
        want = c * ref["dy"] + (prior.double().view(ref["dy"].shape) if prior is not None else 0)
        out["dy"] = frac((dy.double().view(ref["dy"].shape) - want).reshape(B, -1).abs().amax(dim=1), scale)
    if dt is not None:
        out["dt"] = frac((dt.double().view(ref["dy"].shape) + c * ref["dy"]).reshape(B, -1).abs().amax(dim=1), scale)
    if L is not None:
        out["L"] = frac(torch.tensor(abs(float(L) - ref["L"])), torch.tensor(abs(ref["L"])))
    return out


def fp32_fractions(ref):
    return fractions(ref, ref["pix32"], ref["dy32"], L=ref["L32"])


class Worst(dict):
    def take(self, fr):
        for k, v in fr.items():
            self[k] = max(self.get(k, 0.0), v)

    def line(self, label):
        return (f"[sample weight] {label}: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(self.items())) +
                f" of the scale (bar {BAR:.0e})")


def check(ref, pix=None, dy=None, dt=None, worst=None, dy_scale=1.0, prior=None, L=None, label="", accumulate=False):
    """Hold a launch's outputs to THE RULE, and the skipped samples to their contract: pix 0, dt 0, dy 0 on overwrite and
    the prior's bits on accumulate."""
    skip = ~kept(ref["s"])
    B = ref["y"].shape[0]
    clean = ~torch.isnan(ref["s"])
    for name, x in (("pix", pix), ("dy", dy), ("dt", dt)):
        if x is None:
            continue
        assert x.dtype == torch.float32, (label, name)
        rows = x.reshape(B, -1)
        assert not torch.isnan(rows[clean & ~skip]).any(), (label, name, "NaN or not written")
        if name == "dy" and accumulate:
            assert torch.equal(bits(rows[skip]), bits(prior.reshape(B, -1)[skip])), (label, "a skipped sample's dy was touched")
        else:
            assert (rows[skip] == 0).all(), (label, name, "a skipped sample is not exactly 0")
    fr = fractions(ref, pix, dy, dt, dy_scale, prior, L)
    if worst is not None:
        worst.take(fr)
    for name, v in fr.items():
        assert v <= BAR, (label, name, v)
    return fr


# ------------------------------------------------------------------------------------------------------------- the raw calls
P_ = ctypes.c_void_p

PS_BASE = dict(y=1, t=1, B=2, P=64, kind=0, param=0.0, fg_weight=0.0, fg_threshold=0.0, s=1, pix=1, dy=1, dy_scale=1.0,
               accumulate=0, dt=1, max_wgs=None)
# every refusal include/tactilesr_hip.h lists for tsr_pixel_loss_ps_fwd_bwd[_wgs]: the parent's list (its loss and work
# aside), B, P, pix and max_wgs; pointers: 1 = given, 0 = NULL, dt = "dy": the same address as dy
PS_REFUSALS = [(lab, over) for lab, over in PC.REFUSALS if not {"loss", "work", "n"} & set(over)] + [
    ("B 0", dict(B=0)), ("B -1", dict(B=-1)), ("P 0", dict(P=0)), ("P -5", dict(P=-5)), ("P 2^28 + 1", dict(P=(1 << 28) + 1)),
    ("P 2^40", dict(P=1 << 40)), ("null pix", dict(pix=0)), ("max_wgs 0", dict(max_wgs=0)), ("max_wgs -3", dict(max_wgs=-3)),
    ("null y, capped", dict(y=0, max_wgs=4)), ("kind 4, capped", dict(kind=4, max_wgs=4)),
]
PS_ACCEPTED = [("s NULL", dict(s=0)), ("no dy, no dt", dict(dy=0, dt=0)), ("max_wgs 1", dict(max_wgs=1)),
               ("mse param NaN", dict(param=NAN)), ("dy_scale Inf", dict(dy_scale=INF))]


def call_ps(lib, a, y=0, t=0, s=0, pix=0, dy=0, dt=0, stream=0):
    head = (P_(y), P_(t), a["B"], ctypes.c_longlong(a["P"]), a["kind"], ctypes.c_double(a["param"]),
            ctypes.c_float(a["fg_weight"]), ctypes.c_float(a["fg_threshold"]), P_(s), P_(pix), P_(dy),
            ctypes.c_float(a["dy_scale"]), a["accumulate"], P_(dt))
    if a.get("max_wgs") is None:
        return lib.tsr_pixel_loss_ps_fwd_bwd(*head, P_(stream))
    return lib.tsr_pixel_loss_ps_fwd_bwd_wgs(*head, a["max_wgs"], P_(stream))


SSIM_BASE = dict(SC.BASE_ARGS, s=1)
SSIM_REFUSALS = list(SC.REFUSALS)          # tsr_ssim_fwd_bwd_ps refuses what its parent refuses


def call_ssim_ps(lib, a, y=0, t=0, s=0, ssim=0, dy=0, stream=0):
    return lib.tsr_ssim_fwd_bwd_ps(P_(y), P_(t), a["B"], a["H"], a["W"], a["win"], ctypes.c_double(a["sigma"]),
                                   ctypes.c_double(a["C1"]), ctypes.c_double(a["C2"]), P_(s), P_(ssim), P_(dy),
                                   ctypes.c_float(a["dy_scale"]), a["accumulate"], P_(stream))


SCALE_BASE = dict(w=1, B=4, mode=0, s=1, stats=1)
SCALE_REFUSALS = [("null w", dict(w=0)), ("null s", dict(s=0)), ("null stats", dict(stats=0)), ("B 0", dict(B=0)),
                  ("B -1", dict(B=-1)), ("mode -1", dict(mode=-1)), ("mode 2", dict(mode=2)), ("mode 99", dict(mode=99))]


def call_scale(lib, a, w=0, s=0, stats=0, stream=0):
    return lib.tsr_sample_scale(P_(w), a["B"], a["mode"], P_(s), P_(stats), P_(stream))


MEAN_BASE = dict(v=1, s=1, B=4, out=1)
MEAN_REFUSALS = [("null v", dict(v=0)), ("null out", dict(out=0)), ("B 0", dict(B=0)), ("B -7", dict(B=-7))]


def call_mean(lib, a, v=0, s=0, out=0, stream=0):
    return lib.tsr_weighted_mean(P_(v), P_(s), a["B"], P_(out), P_(stream))


def fake_pointers(a, names):
    """Small fake addresses nothing may dereference, 0 for a NULL; "dy" names dy's address."""
    addr = {k: 64 * (i + 1) for i, k in enumerate(names)}
    return {k: (addr["dy"] if a[k] == "dy" else (addr[k] if a[k] else 0)) for k in names}


# ------------------------------------------------------------------------------------------------- the GPU launch harness
GUARD = 64


def placed(n, off=0, fill=None):
    """n floats starting `off` floats past a 16-byte boundary, inside a NaN-filled device buffer with at least GUARD NaNs
    on either side: (buffer, the view, its start in the buffer)."""
    buf = torch.full((n + 2 * GUARD + 4,), NAN, dtype=torch.float32, device="cuda")
    start = GUARD + off
    mid = buf[start:start + n]
    assert mid.data_ptr() % 16 == 4 * off
    if fill is not None:
        mid.copy_(fill.reshape(-1))
    return buf, mid, start


def guards_intact(buf, start, n):
    return bool(torch.isnan(buf[:start]).all() and torch.isnan(buf[start + n:]).all())


def bits(x):
    return x.contiguous().view(torch.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _finish(st, outs, shapes):
    torch.cuda.synchronize()
    assert st == 0, st
    for name, (buf, mid, start) in outs.items():
        assert guards_intact(buf, start, mid.numel()), f"{name} guard band written"
    return {k: v[1].clone().cpu().view(shapes[k]) for k, v in outs.items()}


def _twice(once):
    r1, r2 = once(), once()
    for k in r1:
        assert torch.equal(bits(r1[k]), bits(r2[k])), f"two launches gave different {k} bits"
    return r1


def launch_ps(y, t, s, kind, param=None, fg_weight=0.0, fg_threshold=0.0, want=("pix", "dy", "dt"), dy_scale=1.0,
              accumulate=0, prior=None, offs=(0, 0, 0, 0), max_wgs=None):
    """Two raw tsr_pixel_loss_ps_fwd_bwd[_wgs] launches on CPU inputs y, t (B, ...) and the scale s ((B,) or None = NULL)
    placed between NaN guard bands, outputs prefilled with NaN (dy with `prior` when given); the same bits are required
    of the two.  offs: floats off 16-byte alignment of (y, t, dy, dt)."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    B, n = y.shape[0], y.numel()

    def once():
        _, yd, _ = placed(n, offs[0], y.cuda())
        _, td, _ = placed(n, offs[1], t.cuda())
        sd = placed(B, 0, s.cuda())[1] if s is not None else None
        outs = {}
        for name, size, off in (("pix", B, 0), ("dy", n, offs[2]), ("dt", n, offs[3])):
            if name in want:
                outs[name] = placed(size, off, prior.cuda() if (name == "dy" and prior is not None) else None)
        a = dict(B=B, P=n // B, kind=PC.KIND_CODES[kind], param=param or 0.0, fg_weight=fg_weight, fg_threshold=fg_threshold,
                 dy_scale=dy_scale, accumulate=accumulate, max_wgs=max_wgs)
        st = call_ps(lib, a, y=yd.data_ptr(), t=td.data_ptr(), s=sd.data_ptr() if sd is not None else 0, stream=_stream(),
                     **{k: v[1].data_ptr() for k, v in outs.items()})
        return _finish(st, outs, dict(pix=(B,), dy=tuple(y.shape), dt=tuple(y.shape)))
    return _twice(once)


def launch_ssim(y, t, s, win, sigma, C1, C2, want_dy=True, dy_scale=1.0, accumulate=0, prior=None, parent=False):
    """Two raw tsr_ssim_fwd_bwd_ps launches (`parent`: tsr_ssim_fwd_bwd, which takes no s) in the same harness:
    dict(ssim (B,), dy)."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    B, _, H, W = y.shape

    def once():
        _, yd, _ = placed(y.numel(), 0, y.cuda())
        _, td, _ = placed(y.numel(), 0, t.cuda())
        sd = placed(B, 0, s.cuda())[1] if s is not None else None
        outs = {"ssim": placed(B)}
        if want_dy:
            outs["dy"] = placed(y.numel(), 0, prior.cuda() if prior is not None else None)
        a = dict(B=B, H=H, W=W, win=win, sigma=sigma, C1=C1, C2=C2, dy_scale=dy_scale, accumulate=accumulate)
        ptrs = dict(y=yd.data_ptr(), t=td.data_ptr(), ssim=outs["ssim"][1].data_ptr(),
                    dy=outs["dy"][1].data_ptr() if want_dy else 0, stream=_stream())
        if parent:
            st = SC.call_raw(lib, a, **ptrs)
        else:
            st = call_ssim_ps(lib, a, s=sd.data_ptr() if sd is not None else 0, **ptrs)
        return _finish(st, outs, dict(ssim=(B,), dy=tuple(y.shape)))
    return _twice(once)


def launch_scale(w, norm):
    """Two raw tsr_sample_scale launches: dict(s (B,), stats (2,))."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    B = w.shape[0]

    def once():
        _, wd, _ = placed(B, 0, w.cuda())
        outs = {"s": placed(B), "stats": placed(2)}
        st = call_scale(lib, dict(B=B, mode=NORMS[norm]), w=wd.data_ptr(), s=outs["s"][1].data_ptr(),
                        stats=outs["stats"][1].data_ptr(), stream=_stream())
        return _finish(st, outs, dict(s=(B,), stats=(2,)))
    return _twice(once)


def launch_mean(v, s):
    """Two raw tsr_weighted_mean launches: the (1,) result."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    B = v.shape[0]

    def once():
        _, vd, _ = placed(B, 0, v.cuda())
        sd = placed(B, 0, s.cuda())[1] if s is not None else None
        outs = {"out": placed(1)}
        st = call_mean(lib, dict(B=B), v=vd.data_ptr(), s=sd.data_ptr() if sd is not None else 0,
                       out=outs["out"][1].data_ptr(), stream=_stream())
        return _finish(st, outs, dict(out=(1,)))
    return _twice(once)["out"]


def mean_ref(v, s):
    """fl32((1/B) sum_{s_b != 0} s_b v_b) with the sum in fp64 in index order (python floats)."""
    acc = 0.0
    ss = [1.0] * v.shape[0] if s is None else s.tolist()
    for a, b in zip(ss, v.tolist()):
        if a != 0:
            acc += a * b
    return f32(acc / v.shape[0])
