"""Inputs, case tables, the fp64 restatement with its closed-form gradient, and the checker of the pixel-loss tests
(tsr_pixel_loss_fwd_bwd: MSE / L1 / Charbonnier / Huber of d = y - t with a contact weight).

The yardstick is an fp64 restatement in torch ops:
    w_p = 1 + fg_weight [t_p > fg_threshold]  (on the fp32 values),  loss = (1/n) sum_p w_p rho(d_p),  g = w rho'(d) / n
The bar is the project's parity bar, |kernel - fp64| <= 1e-5 x scale, with the loss itself as the scale of the loss and
the gradient tensor's own max |g| (fp64) as the scale of a gradient.  The rule's second term is not used: the SAME
restatement run in fp32 stays below FP32_BAR = 1e-6 of the scale on every case (asserted on the CPU), so the 1e-5 bar
has a factor of 10 over plain fp32 arithmetic and hides nothing.

Inputs are what the train step sees: sparse non-negative targets (about 10 % of the pixels non-zero), predictions
relu(t + noise); every seventh element is an exact tie y == t (L1's sign(0), Huber's and MSE's exact zero), and a few
elements sit at |d| == delta exactly for both Huber deltas of the table, built from multiples of 2^-6 so that the fp32
difference is exact."""
import ctypes
import functools
import math

import torch

from tactilesr_amd.functional import PIXEL_KINDS as KIND_CODES, PIXEL_LOSS_WORK as WORK      # the codes and the work size of the ABI

BAR = 1e-5
FP32_BAR = 1e-6

# (kind, param): every kind, Charbonnier at the default eps and at one of the noise's size, Huber with most / few of the
# elements in its linear region
KINDS = [("mse", None), ("l1", None), ("charbonnier", 1e-3), ("charbonnier", 0.1), ("huber", 0.25), ("huber", 1.0)]
# (fg_weight, fg_threshold): unweighted; every non-zero target pixel weighted; only the pixels above 0.5 weighted
WEIGHTS = [(0.0, 0.0), (0.0, 0.5), (4.0, 0.0), (4.0, 0.5)]
PARAMS = [(k, p, w, th) for k, p in KINDS for w, th in WEIGHTS]

# The launch's geometry as include/tactilesr_hip.h states it: 256 threads, float4 items, at most WORK workgroups.
assert KIND_CODES == {"mse": 0, "l1": 1, "charbonnier": 2, "huber": 3} and WORK == 2048
STRIDE = WORK * 256 * 4                  # floats the capped grid covers per stride
STRIDE_FACTORS = (1.0, 0.5, 2.0, 0.25)   # the big case's data, scaled per stride: a wrong chunk mapping shows
BIG_N = 3 * STRIDE + 4 * 70000 + 3       # every workgroup walks three strides, 70000 float4 a fourth; 3 floats of tail

# name -> (shape, why)
SIZES = {
    "n1": ((1,), "one element: no whole float4, one thread"),
    "n3": ((3,), "below one float4"),
    "n255": ((255,), "one short of a workgroup's threads"),
    "n256": ((256,), "exactly 64 float4: one wave"),
    "n257": ((257,), "one element of tail"),
    "n1023": ((1023,), "one short of a workgroup of float4, three of tail"),
    "n1025": ((1025,), "one past it"),
    "k1r1": ((4 * 256 * 1 + 1,), "4*256*k + r: a workgroup of float4 and r of tail"),
    "k1r2": ((4 * 256 * 1 + 2,), "r = 2"),
    "k1r3": ((4 * 256 * 1 + 3,), "r = 3"),
    "k3r1": ((4 * 256 * 3 + 1,), "more than one workgroup; the second has one float4 per thread, the first two"),
    "k3r2": ((4 * 256 * 3 + 2,), "r = 2"),
    "k3r3": ((4 * 256 * 3 + 3,), "r = 3"),
    "b2_40": ((2, 1, 40, 40), "the train step's shape at sf 10"),
    "b5_124": ((5, 1, 124, 124), "the largest image of the scale-factor tests, 301 workgroups"),
}
BIG = "big"                                # ((BIG_N,), "three strides of the capped grid plus a ragged fourth")
ALIGN_N = 4 * 256 * 3 + 3                  # the alignment cases: two workgroups of float4 and a tail
DELTAS = (0.25, 1.0)


def make_inputs(shape, seed, stride_factors=None):
    """(y, t) fp32 of `shape`: see the module docstring.  Flat index i: i % 7 == 3 ties; i % 11 == 5 / 8 give
    d = +0.25 / -0.25 and i % 13 == 6 / 10 give d = +1 / -1 (where no tie)."""
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    t = torch.where(torch.rand(n, generator=g) < 0.1, 2 * torch.rand(n, generator=g), torch.zeros(n))
    y = (t + 0.3 * torch.randn(n, generator=g)).clamp_min(0)
    i = torch.arange(n)
    base = (i % 64).float() / 64                                   # multiples of 2^-6 in [0, 1)
    for mod, up, down, delta in ((11, 5, 8, DELTAS[0]), (13, 6, 10, DELTAS[1])):
        m = i % mod == up
        t[m], y[m] = base[m], base[m] + delta                      # d = +delta
        m = i % mod == down
        t[m], y[m] = base[m] + delta, base[m]                      # d = -delta
    tie = i % 7 == 3
    y[tie] = t[tie]
    if stride_factors is not None:
        f = torch.tensor(stride_factors)[(i // STRIDE).clamp_max(len(stride_factors) - 1)]
        y, t = y * f, t * f                                        # powers of two: ties stay ties
    return y.reshape(shape).contiguous(), t.reshape(shape).contiguous()


def f32(x):
    """The fp32 rounding of a Python float, as a Python float (what a c_float argument carries)."""
    return float(torch.tensor(x, dtype=torch.float32))


def weights(t, fg_weight, fg_threshold, dtype):
    """w = 1 + fg_weight [t > fg_threshold], the comparison on the fp32 target against the fp32 threshold."""
    mask = t.detach().float() > torch.tensor(fg_threshold, dtype=torch.float32)
    return 1 + f32(fg_weight) * mask.to(dtype)


def restatement(y, t, kind, param=None, fg_weight=0.0, fg_threshold=0.0):
    """The loss in the tensors' dtype from plain torch ops (differentiable in y and t)."""
    d = y - t
    if kind == "mse":
        rho = d * d
    elif kind == "l1":
        rho = d.abs()
    elif kind == "charbonnier":
        rho = torch.sqrt(d * d + param * param)
    elif kind == "huber":
        a = d.abs()
        rho = torch.where(a <= param, 0.5 * d * d, param * (a - 0.5 * param))
    else:
        raise ValueError(kind)
    return (weights(t, fg_weight, fg_threshold, y.dtype) * rho).sum() / y.numel()


def closed_form(y, t, kind, param=None, fg_weight=0.0, fg_threshold=0.0):
    """d loss / d y in fp64 without autograd: w rho'(d) / n with sign(0) = 0."""
    d = y.double() - t.double()
    if kind == "mse":
        gp = 2 * d
    elif kind == "l1":
        gp = torch.sign(d)
    elif kind == "charbonnier":
        gp = d / torch.sqrt(d * d + param * param)
    else:
        gp = d.clamp(-param, param)
    return weights(t, fg_weight, fg_threshold, torch.float64) * gp / y.numel()


def loss_and_grads(y, t, kind, param, fg_weight, fg_threshold, dtype):
    """(loss, d loss / d y, d loss / d t) of the restatement through autograd in `dtype`."""
    yy, tt = y.detach().to(dtype).clone().requires_grad_(True), t.detach().to(dtype).clone().requires_grad_(True)
    loss = restatement(yy, tt, kind, param, fg_weight, fg_threshold)
    gy, gt = torch.autograd.grad(loss, (yy, tt))
    return loss.detach(), gy, gt


def build_reference(y, t, kind, param, fg_weight, fg_threshold):
    l64, g64, gt64 = loss_and_grads(y, t, kind, param, fg_weight, fg_threshold, torch.float64)
    l32, g32, _ = loss_and_grads(y, t, kind, param, fg_weight, fg_threshold, torch.float32)
    return dict(y=y, t=t, kind=kind, param=param, fg_weight=fg_weight, fg_threshold=fg_threshold, l64=float(l64), g64=g64,
                gt64=gt64, l32=float(l32), g32=g32, scale=float(g64.abs().max()))


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == BIG:
        return make_inputs((BIG_N,), 977, STRIDE_FACTORS)
    if name == "align":
        return make_inputs((ALIGN_N,), 311)
    return make_inputs(SIZES[name][0], 100 + list(SIZES).index(name))


@functools.lru_cache(maxsize=64)
def reference(name, kind, param, fg_weight, fg_threshold):
    """Computed once per (inputs, parameters) and shared; treat as read-only."""
    y, t = inputs(name)
    return build_reference(y, t, kind, param, fg_weight, fg_threshold)


def frac(err, scale):
    """err / scale with 0 / 0 = 0 (an all-tie input has an exactly zero loss and gradient)."""
    return err / scale if scale > 0 else (0.0 if err == 0 else math.inf)


def fp32_fractions(ref):
    """The fp32 restatement's distance from fp64 as fractions of the scale: (loss, gradient)."""
    return (frac(abs(ref["l32"] - ref["l64"]), abs(ref["l64"])),
            frac(float((ref["g32"].double() - ref["g64"]).abs().max()), ref["scale"]))


class Worst:
    """Worst fractions of the scale seen over a table."""

    def __init__(self):
        self.loss = self.grad = 0.0

    def line(self, label):
        return f"[pixel loss] {label}: kernel loss {self.loss:.2e} gradient {self.grad:.2e} of the scale (bar {BAR:.0e})"


def coefficient(ref, dy_scale, contact):
    """fp32 rounding of dy_scale w / n evaluated in fp64 as the header states it: what an L1 element holds."""
    w = 1.0 + (f32(ref["fg_weight"]) if contact else 0.0)
    return f32(f32(dy_scale) * w / ref["y"].numel())


def check(ref, loss, dy=None, dt=None, worst=None, dy_scale=1.0, prior=None, label="", exact=True):
    """Hold the launch's outputs (CPU tensors: loss (1,), dy / dt of y's shape or None) to the bar.  dy is expected as
    prior + dy_scale g, dt as -dy_scale g; the gradient scale is |dy_scale| max |g|, so a prior should be of that
    size.  L1 elements and Huber's linear region must equal the fp32 rounding of +-dy_scale (delta) w / n bit for bit
    (no prior; `exact=False` where autograd has multiplied the launch's output once more), and tie pixels are exactly 0."""
    ev = frac(abs(float(loss) - ref["l64"]), abs(ref["l64"]))
    assert not math.isnan(float(loss)), (label, "NaN loss")
    if worst is not None:
        worst.loss = max(worst.loss, ev)
    assert ev <= BAR, (label, "loss", float(loss), ref["l64"], ev)
    scale = ref["scale"] * abs(f32(dy_scale))
    for name, got, sign in (("dy", dy, 1.0), ("dt", dt, -1.0)):
        if got is None:
            continue
        assert got.dtype == torch.float32 and got.shape == ref["y"].shape, (label, name)
        assert not torch.isnan(got).any(), (label, name, "NaN or an element not written")
        want = sign * f32(dy_scale) * ref["g64"]
        if prior is not None and name == "dy":
            want = want + prior.double()
        eg = frac(float((got.double() - want).abs().max()), scale)
        if worst is not None:
            worst.grad = max(worst.grad, eg)
        assert eg <= BAR, (label, name, eg)
        if prior is not None and name == "dy":
            continue
        d = ref["y"].double() - ref["t"].double()
        assert (got[d == 0] == 0).all(), (label, name, "a tie pixel is not exactly 0")
        if exact and ref["kind"] in ("l1", "huber"):
            delta = 1.0 if ref["kind"] == "l1" else ref["param"]      # the table's deltas are powers of two: exact
            lin = d.abs() > (0.0 if ref["kind"] == "l1" else delta)
            contact = ref["t"] > torch.tensor(ref["fg_threshold"], dtype=torch.float32)
            for c in (False, True):
                sel = lin & (contact == c)
                bits = torch.sign(d[sel]).float() * (sign * delta * coefficient(ref, dy_scale, c))
                assert torch.equal(got[sel], bits), (label, name, "linear region not bit-exact", c)


BASE_ARGS = dict(y=1, t=1, n=100, kind=0, param=0.0, fg_weight=0.0, fg_threshold=0.0, loss=1, dy=1, dy_scale=1.0,
                 accumulate=0, dt=1, work=1)
NAN, INF = float("nan"), float("inf")
# every refusal include/tactilesr_hip.h lists: (label, overrides of BASE_ARGS); pointers: 1 = given, 0 = NULL,
# dt = "dy": the same address as dy
REFUSALS = [
    ("null y", dict(y=0)), ("null t", dict(t=0)), ("null loss", dict(loss=0)), ("null work", dict(work=0)),
    ("n 0", dict(n=0)), ("n -1", dict(n=-1)), ("n -2^40", dict(n=-(1 << 40))),
    ("kind -1", dict(kind=-1)), ("kind 4", dict(kind=4)), ("kind 99", dict(kind=99)),
    ("charbonnier eps 0", dict(kind=2, param=0.0)), ("charbonnier eps -1", dict(kind=2, param=-1.0)),
    ("charbonnier eps NaN", dict(kind=2, param=NAN)), ("charbonnier eps Inf", dict(kind=2, param=INF)),
    ("huber delta 0", dict(kind=3, param=0.0)), ("huber delta -1", dict(kind=3, param=-1.0)),
    ("huber delta NaN", dict(kind=3, param=NAN)), ("huber delta Inf", dict(kind=3, param=INF)),
    ("fg_weight -1", dict(fg_weight=-1.0)), ("fg_weight NaN", dict(fg_weight=NAN)), ("fg_weight Inf", dict(fg_weight=INF)),
    ("fg_threshold NaN", dict(fg_threshold=NAN)),
    ("accumulate 2", dict(accumulate=2)), ("accumulate -1", dict(accumulate=-1)),
    ("accumulate without dy", dict(accumulate=1, dy=0)), ("accumulate without dy, dt given", dict(accumulate=1, dy=0, dt=1)),
    ("dy_scale NaN", dict(dy_scale=NAN)), ("dy_scale NaN, no dy", dict(dy_scale=NAN, dy=0, dt=0)),
    ("dt is dy", dict(dt="dy")),
]
# what a refusal table must not refuse (status 0 on the GPU): the MSE and L1 do not read param
ACCEPTED = [("mse param NaN", dict(kind=0, param=NAN)), ("l1 param -1", dict(kind=1, param=-1.0)),
            ("no dy, no dt", dict(dy=0, dt=0)), ("fg_threshold -Inf", dict(fg_threshold=-INF, fg_weight=2.0))]


def call_raw(lib, a, y=0, t=0, loss=0, dy=0, dt=0, work=0, stream=0):
    """tsr_pixel_loss_fwd_bwd with the scalars of `a` and the given addresses; returns the status."""
    P = ctypes.c_void_p
    return lib.tsr_pixel_loss_fwd_bwd(P(y), P(t), ctypes.c_longlong(a["n"]), a["kind"], ctypes.c_double(a["param"]),
                                      ctypes.c_float(a["fg_weight"]), ctypes.c_float(a["fg_threshold"]), P(loss), P(dy),
                                      ctypes.c_float(a["dy_scale"]), a["accumulate"], P(dt), P(work), P(stream))
