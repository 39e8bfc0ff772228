"""The yardstick, the data, the case tables, the checker and the launch harness of the contact-readout tests
(tsr_contact_readout, csrc/contact_readout.hip).  Nothing at import time touches a device: tests/test_contact_cpu.py
checks every precondition the GPU tests (tests/test_gpu_contact.py) rely on.

THE RESTATEMENT is the record and the pair of include/tactilesr_hip.h written the textbook way in fp64 numpy: the masked,
intensity-weighted centroid first, then the central moments about it (two passes), atan2 and the eigenvalues.  It shares
no intermediate with the kernel, which sums integer offsets about the peak pixel and moves them to the centroid.

THE BARS are the project's own 1e-5 x scale:
    counts (record 0; pair 0, 1) and tau             bit-equal
    area, mass, total, peak                          1e-5 x their own magnitude
    positions, centroid, axes, distances             1e-5 x span (rows: span_r, columns: span_c, mixed: the smaller)
    second moments                                   1e-5 x span^2
    IoU, Dice, mass_rel_err                          1e-5 x max(1, value)
    theta, angle_diff                                1e-5 rad where (lambda+ - lambda-) / lambda+ >= 0.05
The area is an exact count times a constant, so it takes the bar of the masses.  theta is the angle of an axis, so two
angles are compared modulo pi (-pi/2 + e and pi/2 - e are 2e apart); the range (-pi/2, pi/2] is asserted on its own.  On
a more isotropic image theta is only required to be finite and in range; a contact without extent (one pixel: all three
moments exactly 0) must give exactly 0.  The NaN pattern of a record must equal the restatement's.

THE DATA are multiples of 2^-10: every sum of pixels is exact in fp64 in any order, a pixel either equals tau exactly (a
tie the strict comparison excludes; tau is then exactly representable) or is far from it -- `margin_ok` is that
condition, 1e-6 (mx - mn), and the CPU test asserts it for every case -- and peaks tie, which exercises the
first-maximum rule."""
import ctypes
import math

import numpy as np
import torch

NAN, INF = float("nan"), float("inf")
BAR = 1e-5
ANISO = 0.05
REC, PAIR, MAX_WGS = 16, 8, 2048          # TSR_CONTACT_REC, TSR_CONTACT_PAIR, TSR_CONTACT_MAX_WGS
MODES = {"abs": 0, "range": 1}
Q = 1024.0                                # the data grid: multiples of 2^-10

SHAPES = [(1, 1), (1, 5), (4, 4), (5, 7), (3, 127), (128, 4), (40, 40), (100, 100), (160, 160)]
BATCHES = (1, 7, 67)
THRESHOLDS = [(m, t) for m in ("abs", "range") for t in (0.0, 0.3, 0.5)]
GAINS = (1.0, 10.0)
SPANS = ((4.0, 4.0), (4.0, 6.0))


# ---------------------------------------------------------------------------------------------------------- the restatement
def analyse(img, mode, thr, gain=1.0, span=(4.0, 4.0)):
    """img (B,H,W) float32 -> (record (B,16) float64, mask (B,H*W) bool, bad (B,) bool)."""
    img = np.asarray(img, dtype=np.float32)
    B, H, W = img.shape
    flat = img.reshape(B, -1).astype(np.float64)
    bad = ~np.isfinite(flat).all(axis=1)
    v = np.where(bad[:, None], 0.0, flat)
    mn, mx = v.min(axis=1), v.max(axis=1)
    if mode == "abs":
        tau = np.full(B, float(np.float32(thr)))
    else:
        tau = mn + thr * (mx - mn)                                  # numpy: a product, then a sum
    m = v > tau[:, None]
    u = (np.arange(H) + 0.5) * span[0] / H - 0.5
    c = (np.arange(W) + 0.5) * span[1] / W - 0.5
    U, V = np.repeat(u, W)[None], np.tile(c, H)[None]
    n = m.sum(axis=1)
    first = v.argmax(axis=1)                                        # the first maximum in row-major order
    w = np.where(m, v, 0.0)
    M0 = w.sum(axis=1)
    ok = (n > 0) & (M0 > 0)
    D = np.where(ok, M0, 1.0)
    cu, cv = (w * U).sum(axis=1) / D, (w * V).sum(axis=1) / D
    du, dv = U - cu[:, None], V - cv[:, None]
    muu, mvv, muv = (w * du * du).sum(axis=1) / D, (w * dv * dv).sum(axis=1) / D, (w * du * dv).sum(axis=1) / D
    one = ok & (n == 1)                                             # a single pixel IS its centroid: (v u) / v may miss u
    only = m.argmax(axis=1)
    cu, cv = np.where(one, U[0][only], cu), np.where(one, V[0][only], cv)
    muu, mvv, muv = np.where(one, 0.0, muu), np.where(one, 0.0, mvv), np.where(one, 0.0, muv)
    a2, a1 = 2.0 * muv, muu - mvv
    th = np.where((a2 == 0) & (a1 == 0), 0.0, 0.5 * np.arctan2(a2, a1))
    th = np.where(th <= -math.pi / 2, math.pi / 2, th)
    h, d = 0.5 * (muu + mvv), np.sqrt((0.5 * a1) ** 2 + muv ** 2)
    rec = np.stack([n.astype(np.float64), n * (span[0] / H) * (span[1] / W), gain * M0, gain * v.sum(axis=1), gain * mx,
                    U[0][first], V[0][first], cu, cv, muu, mvv, muv, th, np.sqrt(np.maximum(h + d, 0.0)),
                    np.sqrt(np.maximum(h - d, 0.0)), tau], axis=1)
    rec[~ok, 7:15] = NAN
    rec[bad] = NAN
    return rec, m, bad


def record(img, mode, thr, gain=1.0, span=(4.0, 4.0)):
    return analyse(img, mode, thr, gain, span)[0]


def pair(y, t, mode, thr, gain=1.0, span=(4.0, 4.0)):
    """(pair (B,8), record_y, record_t), float64."""
    ry, my, by = analyse(y, mode, thr, gain, span)
    rt, mt, bt = analyse(t, mode, thr, gain, span)
    inter = (my & mt).sum(axis=1).astype(np.float64)
    ny, nt = my.sum(axis=1).astype(np.float64), mt.sum(axis=1).astype(np.float64)
    uni = ny + nt - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 1.0)
        dice = np.where(ny + nt > 0, 2 * inter / np.where(ny + nt > 0, ny + nt, 1.0), 1.0)
        dist = np.hypot(ry[:, 7] - rt[:, 7], ry[:, 8] - rt[:, 8])
        Mt = rt[:, 2]
        okm = (nt > 0) & (Mt > 0)
        rel = np.where(okm, np.abs(ry[:, 2] - Mt) / np.where(okm, Mt, 1.0), NAN)
        pk = np.hypot(ry[:, 5] - rt[:, 5], ry[:, 6] - rt[:, 6])
        dth = np.abs(ry[:, 12] - rt[:, 12])
        dth = np.where(dth > math.pi / 2, math.pi - dth, dth)
    out = np.stack([inter, uni, iou, dice, dist, rel, pk, dth], axis=1)
    out[by | bt] = NAN
    return out, ry, rt


def brute_force(img, mode, thr, gain=1.0, span=(4.0, 4.0)):
    """The record of ONE finite (H,W) image by explicit double loops over python floats."""
    H, W = img.shape
    px = [[float(img[x, c]) for c in range(W)] for x in range(H)]
    mn = min(min(r) for r in px)
    mx = max(max(r) for r in px)
    tau = float(np.float32(thr)) if mode == "abs" else mn + thr * (mx - mn)
    uc = lambda x: (x + 0.5) * span[0] / H - 0.5
    vc = lambda c: (c + 0.5) * span[1] / W - 0.5
    n, M0, tot, pk = 0, 0.0, 0.0, None
    for x in range(H):
        for c in range(W):
            tot += px[x][c]
            if pk is None and px[x][c] == mx:
                pk = (uc(x), vc(c))
            if px[x][c] > tau:
                n += 1
                M0 += px[x][c]
    out = [float(n), n * (span[0] / H) * (span[1] / W), gain * M0, gain * tot, gain * mx, pk[0], pk[1]] + [NAN] * 8 + [tau]
    if n == 1 and M0 > 0:                                           # a single pixel is its own centroid, exactly
        at = [(uc(x), vc(c)) for x in range(H) for c in range(W) if px[x][c] > tau][0]
        out[7:15] = [at[0], at[1], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    elif n > 0 and M0 > 0:
        cu = sum(px[x][c] * uc(x) for x in range(H) for c in range(W) if px[x][c] > tau) / M0
        cv = sum(px[x][c] * vc(c) for x in range(H) for c in range(W) if px[x][c] > tau) / M0
        muu = sum(px[x][c] * (uc(x) - cu) ** 2 for x in range(H) for c in range(W) if px[x][c] > tau) / M0
        mvv = sum(px[x][c] * (vc(c) - cv) ** 2 for x in range(H) for c in range(W) if px[x][c] > tau) / M0
        muv = sum(px[x][c] * (uc(x) - cu) * (vc(c) - cv) for x in range(H) for c in range(W) if px[x][c] > tau) / M0
        th = 0.0 if (muv == 0 and muu == mvv) else 0.5 * math.atan2(2 * muv, muu - mvv)
        if th <= -math.pi / 2:
            th = math.pi / 2
        h, d = 0.5 * (muu + mvv), math.sqrt((0.5 * (muu - mvv)) ** 2 + muv ** 2)
        out[7:15] = [cu, cv, muu, mvv, muv, th, math.sqrt(max(h + d, 0.0)), math.sqrt(max(h - d, 0.0))]
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------------ the data
def quantise(img):
    return (np.round(np.asarray(img, dtype=np.float64) * Q) / Q).astype(np.float32)


def _settle(img):
    """Keep the range off the multiples of 10 grid steps (0.3 x range then lands 0.1 .. 0.9 of a step from the grid):
    the first maximum of such an image is raised by one step."""
    flat = img.reshape(img.shape[0], -1)
    for b in range(flat.shape[0]):
        k = int(round((float(flat[b].max()) - float(flat[b].min())) * Q))
        if k % 10 == 0 and k > 0:
            flat[b, int(flat[b].argmax())] += 1.0 / Q
    return img


def blobs(B, H, W, seed, signed=False):
    """B anisotropic Gaussian blobs (axis ratio 2.5 .. 4, amplitude 0.8 .. 1.6, any angle, centre in the middle half) on
    an exactly zero background, quantised; `signed` subtracts a second, weaker blob elsewhere."""
    g = np.random.default_rng(seed)
    x = (np.arange(H) + 0.5)[None, :, None]
    c = (np.arange(W) + 0.5)[None, None, :]

    def one(amp):
        cx, cc = (0.25 + 0.5 * g.random(B)) * H, (0.25 + 0.5 * g.random(B)) * W
        minor = np.maximum(0.04 * min(H, W) * (1 + g.random(B)), 0.45)
        major = minor * (2.5 + 1.5 * g.random(B))
        ang = g.random(B) * math.pi
        if H < 8 * W and W < 8 * H:
            ca, sa = np.cos(ang), np.sin(ang)
        else:                                                       # a strip: the long axis along the strip
            ca, sa = (np.zeros(B), np.ones(B)) if W > H else (np.ones(B), np.zeros(B))
            major = np.minimum(major * 4, 0.2 * max(H, W))
        dx, dc = x - cx[:, None, None], c - cc[:, None, None]
        p = dx * ca[:, None, None] + dc * sa[:, None, None]
        q = -dx * sa[:, None, None] + dc * ca[:, None, None]
        return amp[:, None, None] * np.exp(-0.5 * ((p / major[:, None, None]) ** 2 + (q / minor[:, None, None]) ** 2))
    img = one(0.8 + 0.8 * g.random(B))
    if signed:
        img = img - one(0.3 + 0.3 * g.random(B))
    return _settle(quantise(img))


def rectangle(H, W, r0, r1, c0, c1, value=1.0):
    img = np.zeros((1, H, W), dtype=np.float32)
    img[0, r0:r1, c0:c1] = value
    return img


def impulses(H, W, points):
    """One image; points = [(row, column, value)]."""
    img = np.zeros((1, H, W), dtype=np.float32)
    for x, c, v in points:
        img[0, x, c] = v
    return img


def margin_ok(img, mode, thr):
    """No pixel within 1e-6 (mx - mn) of its image's tau unless it EQUALS a tau that is exactly representable in fp32."""
    img = np.asarray(img, dtype=np.float32)
    v = img.reshape(img.shape[0], -1).astype(np.float64)
    mn, mx = v.min(axis=1), v.max(axis=1)
    tau = np.full(len(v), float(np.float32(thr))) if mode == "abs" else mn + thr * (mx - mn)
    exact = tau.astype(np.float32).astype(np.float64) == tau
    near = np.abs(v - tau[:, None]) <= 1e-6 * (mx - mn)[:, None]
    tie = (v == tau[:, None]) & exact[:, None]
    return bool((~near | tie).all())


def shape_images(H, W, B):
    """The (y, t) of the shape table: t another blob set, so the pair entries are non-trivial."""
    return blobs(B, H, W, seed=1000 * H + W + B), blobs(B, H, W, seed=77 + 1000 * H + W + B)


def theta_checked(rec64):
    """Per image: True where theta is held to 1e-5 (anisotropic) or to an exact 0 (a contact without extent: all three
    moments exactly 0)."""
    lp, lm = rec64[:, 13] ** 2, rec64[:, 14] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        aniso = np.where(lp > 0, (lp - lm) / np.where(lp > 0, lp, 1.0), 0.0) >= ANISO
    point = (rec64[:, 9] == 0) & (rec64[:, 10] == 0) & (rec64[:, 11] == 0)
    return aniso | point, aniso


# ------------------------------------------------------------------------------------------------------------- the checker
def bits(x):
    return x.contiguous().view(torch.int32)


def _f32bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


class Worst(dict):
    def take(self, name, v):
        if v == v:
            self[name] = max(self.get(name, 0.0), float(v))

    def line(self, what):
        return f"[contact] {what}: worst fraction of the bar " + ", ".join(f"{k} {v:.2e}" for k, v in self.items())


def _held(got, ref, scale, name, worst, label):
    """|got - ref| <= BAR x scale elementwise on the finite entries; the NaN patterns must agree."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert (np.isnan(got) == np.isnan(ref)).all(), (label, name, "NaN pattern")
    fin = ~np.isnan(ref)
    if not fin.any():
        return
    err = np.abs(got[fin] - ref[fin])
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), ref.shape)[fin]
    zero = sc == 0
    assert (err[zero] == 0).all(), (label, name, "an exact zero")
    if (~zero).any():
        frac = float((err[~zero] / (BAR * sc[~zero])).max())
        if worst is not None:
            worst.take(name, frac)
        assert frac <= 1.0, (label, name, frac)


def check_record(got, ref, span, worst=None, label=""):
    """got (B,16) float32 (numpy or torch), ref (B,16) float64."""
    got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (label, got.dtype, got.shape)
    sr, sc, sm = span[0], span[1], min(span)
    for i in (0, 15):                                               # counts and tau: bit-equal
        nan = np.isnan(ref[:, i])
        assert (np.isnan(got[:, i]) == nan).all(), (label, i, "NaN pattern")
        assert (_f32bits(got[~nan, i]) == _f32bits(ref[~nan, i])).all(), (label, i, "bits")
    for i, name in ((1, "area"), (2, "mass"), (3, "total"), (4, "peak")):
        _held(got[:, i], ref[:, i], np.abs(ref[:, i]), name, worst, label)
    for i, s in ((5, sr), (6, sc), (7, sr), (8, sc), (13, sm), (14, sm)):
        _held(got[:, i], ref[:, i], s, "position", worst, label)
    for i, s in ((9, sr * sr), (10, sc * sc), (11, sr * sc)):
        _held(got[:, i], ref[:, i], s, "moment", worst, label)
    th, rth = got[:, 12].astype(np.float64), ref[:, 12]
    assert (np.isnan(th) == np.isnan(rth)).all(), (label, "theta NaN pattern")
    have = ~np.isnan(rth)
    assert ((th[have] > -np.float32(math.pi / 2)) & (th[have] <= np.float32(math.pi / 2))).all(), (label, "theta range")
    _, aniso = theta_checked(ref)
    flat = have & (ref[:, 9] == 0) & (ref[:, 10] == 0) & (ref[:, 11] == 0)      # not lambda+ == 0: signed weights clamp
    assert (th[flat] == 0).all(), (label, "theta of a contact without extent")
    sel = have & aniso
    if sel.any():
        d = np.abs(th[sel] - rth[sel])
        d = np.minimum(d, math.pi - d)                              # an axis: modulo pi
        if worst is not None:
            worst.take("theta", float(d.max()) / BAR)
        assert float(d.max()) <= BAR, (label, "theta", float(d.max()))


def check_pair(got, ref, ry, rt, span, worst=None, label=""):
    got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (label, got.dtype, got.shape)
    fin = ~np.isnan(ref[:, 0])
    assert (np.isnan(got[:, :2]) == np.isnan(ref[:, :2])).all(), (label, "count NaN pattern")
    for i in (0, 1):
        assert (_f32bits(got[fin, i]) == _f32bits(ref[fin, i])).all(), (label, "pair count", i)
    for i, name in ((2, "iou"), (3, "dice"), (5, "mass_rel_err")):
        _held(got[:, i], ref[:, i], np.maximum(1.0, np.abs(np.nan_to_num(ref[:, i]))), name, worst, label)
    for i in (4, 6):
        _held(got[:, i], ref[:, i], min(span), "distance", worst, label)
    d, rd = got[:, 7].astype(np.float64), ref[:, 7]
    assert (np.isnan(d) == np.isnan(rd)).all(), (label, "angle_diff NaN pattern")
    have = ~np.isnan(rd)
    assert ((d[have] >= 0) & (d[have] <= np.float32(math.pi / 2))).all(), (label, "angle_diff range")
    sel = have & theta_checked(ry)[1] & theta_checked(rt)[1]
    if sel.any():
        e = np.abs(d[sel] - rd[sel])
        if worst is not None:
            worst.take("angle_diff", float(e.max()) / BAR)
        assert float(e.max()) <= BAR, (label, "angle_diff", float(e.max()))


# ------------------------------------------------------------------------------------------------------------- the raw call
BASE_ARGS = dict(y=1, t=1, B=2, H=8, W=8, mode=0, threshold=0.25, gain=1.0, span_r=4.0, span_c=4.0, rec_y=1, rec_t=1,
                 pair=1, max_wgs=None)
# every refusal include/tactilesr_hip.h lists: (label, overrides of BASE_ARGS).  Pointers: 1 = given, 0 = NULL, a name =
# the address of that buffer, "name+" = 4 floats into it (overlapping, not equal)
REFUSALS = [
    ("null y", dict(y=0)), ("null rec_y", dict(rec_y=0)), ("null y, single", dict(y=0, t=0, rec_t=0, pair=0)),
    ("B 0", dict(B=0)), ("B -1", dict(B=-1)), ("H 0", dict(H=0)), ("W 0", dict(W=0)), ("H -3", dict(H=-3)), ("W -1", dict(W=-1)),
    ("H W 2^24 + 1", dict(H=(1 << 24) + 1, W=1)), ("H W 4097 x 4096", dict(H=4097, W=4096)),
    ("H W overflowing int", dict(H=1 << 16, W=1 << 16)),
    ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)),
    ("threshold NaN", dict(threshold=NAN)), ("threshold Inf", dict(threshold=INF)), ("threshold -Inf", dict(threshold=-INF)),
    ("range threshold 1", dict(mode=1, threshold=1.0)), ("range threshold -0.1", dict(mode=1, threshold=-0.1)),
    ("range threshold 2", dict(mode=1, threshold=2.0)), ("range threshold NaN", dict(mode=1, threshold=NAN)),
    ("gain NaN", dict(gain=NAN)), ("gain Inf", dict(gain=INF)), ("gain -Inf", dict(gain=-INF)),
    ("span_r 0", dict(span_r=0.0)), ("span_r -4", dict(span_r=-4.0)), ("span_r NaN", dict(span_r=NAN)),
    ("span_r Inf", dict(span_r=INF)), ("span_c 0", dict(span_c=0.0)), ("span_c -4", dict(span_c=-4.0)),
    ("span_c NaN", dict(span_c=NAN)), ("span_c Inf", dict(span_c=INF)),
    ("no t, rec_t given", dict(t=0, pair=0)), ("no t, pair given", dict(t=0, rec_t=0)), ("no t, both given", dict(t=0)),
    ("t without pair", dict(pair=0)), ("t without pair or rec_t", dict(pair=0, rec_t=0)),
    ("rec_y is y", dict(rec_y="y")), ("rec_y inside y", dict(rec_y="y+")), ("rec_y is t", dict(rec_y="t")),
    ("rec_t is y", dict(rec_t="y")), ("rec_t inside t", dict(rec_t="t+")), ("pair is y", dict(pair="y")),
    ("pair inside t", dict(pair="t+")), ("rec_t is rec_y", dict(rec_t="rec_y")), ("rec_t inside rec_y", dict(rec_t="rec_y+")),
    ("pair is rec_y", dict(pair="rec_y")), ("pair inside rec_t", dict(pair="rec_t+")),
    ("max_wgs 0", dict(max_wgs=0)), ("max_wgs -5", dict(max_wgs=-5)),
]
# what the table must not refuse (status 0 on the GPU)
ACCEPTED = [
    ("single form", dict(t=0, rec_t=0, pair=0)), ("pair without rec_t", dict(rec_t=0)), ("t is y", dict(t="y")),
    ("gain 0", dict(gain=0.0)), ("gain -2", dict(gain=-2.0)), ("a negative abs threshold", dict(threshold=-3.0)),
    ("range threshold 0", dict(mode=1, threshold=0.0)), ("abs threshold 7", dict(threshold=7.0)),
    ("max_wgs 1", dict(max_wgs=1)), ("span 1e-3 x 1e3", dict(span_r=1e-3, span_c=1e3)),
]
PTRS = ("y", "t", "rec_y", "rec_t", "pair")


def resolve_ptrs(a, addr):
    """The five addresses of a call: `addr` holds each buffer's own address."""
    out = {}
    for k in PTRS:
        v = a[k]
        if isinstance(v, str):
            out[k] = addr[v.rstrip("+")] + (16 if v.endswith("+") else 0)
        else:
            out[k] = addr[k] if v else 0
    return out


def call_raw(lib, a, y=0, t=0, rec_y=0, rec_t=0, pair=0, stream=0):
    """tsr_contact_readout (a["max_wgs"] None) or tsr_contact_readout_wgs with the scalars of `a` and the given
    addresses; returns the status."""
    P, D = ctypes.c_void_p, ctypes.c_double
    head = (P(y), P(t), a["B"], a["H"], a["W"], a["mode"], D(a["threshold"]), D(a["gain"]), D(a["span_r"]),
            D(a["span_c"]), P(rec_y), P(rec_t), P(pair))
    if a.get("max_wgs") is None:
        return lib.tsr_contact_readout(*head, P(stream))
    return lib.tsr_contact_readout_wgs(*head, a["max_wgs"], P(stream))


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
        mid.copy_(torch.as_tensor(fill).reshape(-1))
    return buf, mid, start


def guards_intact(buf, start, n):
    return bool(torch.isnan(buf[:start]).all() and torch.isnan(buf[start + n:]).all())


def _launch_once(lib, y, t, mode, thr, gain, span, want, offs, max_wgs):
    B, H, W = y.shape
    _, yd, _ = placed(y.size, offs.get("y", 0), torch.from_numpy(y))
    td = None
    if t is not None:
        td = yd if t is y else placed(t.size, offs.get("t", 0), torch.from_numpy(t))[1]
    sizes = dict(rec_y=REC * B, rec_t=REC * B, pair=PAIR * B)
    outs = {k: placed(sizes[k], offs.get(k, 0)) for k in want}
    a = dict(B=B, H=H, W=W, mode=MODES[mode], threshold=thr, gain=gain, span_r=span[0], span_c=span[1], max_wgs=max_wgs)
    st = call_raw(lib, a, y=yd.data_ptr(), t=td.data_ptr() if td is not None else 0,
                  stream=torch.cuda.current_stream().cuda_stream, **{k: v[1].data_ptr() for k, v in outs.items()})
    torch.cuda.synchronize()
    assert st == 0, st
    for name, (buf, mid, start) in outs.items():
        assert guards_intact(buf, start, mid.numel()), f"{name} guard band written"
    return {k: v[1].clone().cpu().view(B, -1) for k, v in outs.items()}


def launch(y, t, mode, thr, gain=1.0, span=(4.0, 4.0), want=None, offs=None, max_wgs=None):
    """Two raw launches on numpy (B,H,W) float32 inputs placed between NaN guard bands, every output prefilled with NaN
    between guard bands; the two must give the same bits; the outputs come back as a dict of CPU tensors.  `t is y` passes
    one buffer twice.  offs: {name: floats off 16-byte alignment}."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    if want is None:
        want = ("rec_y",) if t is None else ("rec_y", "rec_t", "pair")
    r1 = _launch_once(lib, y, t, mode, thr, gain, span, want, offs or {}, max_wgs)
    r2 = _launch_once(lib, y, t, mode, thr, gain, span, want, offs or {}, max_wgs)
    for k in r1:
        assert torch.equal(bits(r1[k]), bits(r2[k])), f"two launches gave different {k} bits"
    return r1


def assert_bits(a, b, what=""):
    """Two tensors with the same bits; a failure names the first entries that differ."""
    if not torch.equal(bits(a), bits(b)):
        at = (bits(a) != bits(b)).nonzero()[:4].tolist()
        raise AssertionError((what, [(i, float(a[tuple(i)]), float(b[tuple(i)])) for i in at]))


def same_bits(a, b, what=""):
    assert set(a) == set(b), (what, set(a), set(b))
    for k in a:
        assert_bits(a[k], b[k], (what, k))
