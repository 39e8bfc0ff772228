"""Cases, restatements, checker and launch harness of the taxel sensor-noise kernel (tsr_taxel_noise, csrc/taxel_noise.hip).

Everything here is written from the contract in include/tactilesr_hip.h without reading ``tactilesr_amd.functional``:
Philox4x32-10 in numpy (vectorised, 32-bit values held in uint64), the formulas in fp64 and in plain fp32, the case
tables with the reason for every case, the checker, and the guarded launch (NaN-prefilled output between NaN guard bands,
run twice).  A spec is a plain dict: ``axis_cnt``, ``sigma_add`` / ``sigma_mul`` (lists of axis_cnt), ``gain_jitter``,
``drop_thresh`` (the integer), ``drop_value``.
"""
import ctypes

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
NAN_BITS = 0x7fc00000
TWO24 = 1 << 24

# (counter, key, output): the known answers of Philox4x32-10
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(counter, key):
    """Ten rounds on four broadcastable counter arrays and two key words: the four output arrays (uint64 holding 32 bits)."""
    u = np.uint64
    mask = u(0xffffffff)
    c = [np.asarray(x, dtype=np.uint64) & mask for x in counter]
    k = [u(int(key[0]) & 0xffffffff), u(int(key[1]) & 0xffffffff)]
    for _ in range(10):
        p0 = u(M0) * c[0]                                              # 32 x 32 bits: fits 64
        p1 = u(M1) * c[2]
        c = [(p1 >> u(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> u(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + u(W0)) & mask, (k[1] + u(W1)) & mask]
    return c


def words(ids, blocks, tag, seed, offset):
    """(B, 4 * blocks) uint32: lane l of block j of effect ``tag`` is item 4 j + l.  Counter (block, id, offset, tag), key
    (seed_lo, seed_hi)."""
    ids = np.asarray(ids, dtype=np.int64)
    assert ((ids >= 0) & (ids < 2 ** 31)).all()
    j = np.arange(blocks, dtype=np.uint64)[None, :]
    i = ids.astype(np.uint64)[:, None]
    seed = int(seed) % (1 << 64)
    r = philox((j, i, np.uint64(offset), np.uint64(tag)), (seed & 0xffffffff, seed >> 32))
    r = [np.broadcast_to(x, (len(ids), blocks)) for x in r]
    return np.stack(r, axis=-1).reshape(len(ids), 4 * blocks).astype(np.uint32)


def _quarter_split(a, dt):
    """a in [0, 2) on a grid of 2^-23 -> (quarter index 0..4, remainder in [-1/4, 1/4]), both exact in fp32 and fp64."""
    k = np.floor(a * dt(2) + dt(0.5))
    return k.astype(np.int64) & 3, (a - k * dt(0.5)).astype(dt)


def normals(w, dt):
    """Unit normals of the noise words w (B, 4 nb) in precision ``dt``: words (r0, r1) of a block give items 4 j (cos) and
    4 j + 1 (sin), words (r2, r3) items 4 j + 2 and 4 j + 3.  cos(pi a) / sin(pi a) take the quarter off exactly first, as
    any cospi / sinpi does: what is left is one rounding of pi r."""
    B = w.shape[0]
    p = w.reshape(B, -1, 2, 2)
    ra, rb = p[..., 0], p[..., 1]
    u1 = ((2 * (ra >> 9).astype(np.int64) + 1).astype(dt) * dt(2.0 ** -24)).astype(dt)
    a = ((rb >> 8).astype(dt) * dt(2.0 ** -23)).astype(dt)              # 2 u2
    R = np.sqrt(dt(-2) * np.log(u1)).astype(dt)
    q, r = _quarter_split(a, dt)
    t = (dt(np.pi) * r).astype(dt)
    c, s = np.cos(t).astype(dt), np.sin(t).astype(dt)
    cosv = np.choose(q, [c, -s, -c, s])
    sinv = np.choose(q, [s, c, -s, -c])
    return np.stack([R * cosv, R * sinv], axis=-1).astype(dt).reshape(B, -1)


def gain32(w, gain_jitter):
    """g = fmaf(gain_jitter, 2 u - 1, 1) as the fp32 number the contract defines: 2 u - 1 is exact, the product of two
    24-bit numbers is exact in fp64, and for gain_jitter >= 2^-20 so is its sum with 1; one rounding to fp32 remains."""
    assert gain_jitter == 0 or abs(gain_jitter) >= 2.0 ** -20
    u2m1 = 2.0 * ((w >> 8).astype(np.float64) * 2.0 ** -24) - 1.0
    return (1.0 + np.float64(np.float32(gain_jitter)) * u2m1).astype(np.float32)


def restate(x, spec, seed, offset, ids, dt=np.float64):
    """The contract on x (B, C, H, W) fp32 numpy, in precision ``dt`` (fp64: every step exact-ish; fp32: plain numpy fp32
    operations, one rounding each, no fma).  ids: int array of B valid ids.  Returns a dict: y (the output before dropout, dt), v (after
    gain, dt), s (the noise sigma per element, dt; 0 where the axis is neutral), active (bool per element: noise applied),
    dead (B, P bool), n (the normals, dt)."""
    B, C, H, W = x.shape
    P, a = H * W, spec["axis_cnt"]
    assert C % a == 0
    xr = x.reshape(B, C // a, a, P)
    with np.errstate(invalid="ignore", over="ignore"):
        if spec["gain_jitter"] != 0:
            w = words(ids, (a * P + 3) // 4, 1, seed, offset)[:, :a * P].reshape(B, 1, a, P)
            if dt is np.float64:
                u2m1 = 2.0 * ((w >> 8).astype(np.float64) * 2.0 ** -24) - 1.0
                g = 1.0 + np.float64(np.float32(spec["gain_jitter"])) * u2m1
            else:
                u = (w >> 8).astype(np.float32) * np.float32(2.0 ** -24)
                g = np.float32(1) + np.float32(spec["gain_jitter"]) * (np.float32(2) * u - np.float32(1))
            v = (g * xr.astype(dt)).astype(dt)
        else:
            v = xr.astype(dt)
        sa = np.asarray(spec["sigma_add"], dtype=np.float32).astype(dt).reshape(1, 1, a, 1)
        sm = np.asarray(spec["sigma_mul"], dtype=np.float32).astype(dt).reshape(1, 1, a, 1)
        active = np.broadcast_to((sa != 0) | (sm != 0), v.shape)
        nb = (C * P + 3) // 4
        n = normals(words(ids, nb, 0, seed, offset), dt)[:, :C * P].reshape(v.shape)
        t = (sm * v).astype(dt)
        s = np.where(active, np.sqrt((t * t + sa * sa).astype(dt)), dt(0)).astype(dt)
        y = np.where(active, (v + (s * n).astype(dt)).astype(dt), v)
    dead = np.zeros((B, P), dtype=bool)
    if spec["drop_thresh"] != 0:
        dead = (words(ids, (P + 3) // 4, 2, seed, offset)[:, :P] >> 8).astype(np.int64) < spec["drop_thresh"]
    shape = (B, C, H, W)
    return dict(y=y.reshape(shape), v=v.reshape(shape), s=s.reshape(shape), active=active.reshape(shape), dead=dead,
                n=n.reshape(shape))


def apply_dropout(y32, dead, drop_value):
    """The select: a dead taxel reads drop_value in every channel."""
    B, C, H, W = y32.shape
    return np.where(dead.reshape(B, 1, H, W), np.float32(drop_value), y32)


# ---- specs: why each is in the table
def spec(sigma_add=0.0, sigma_mul=0.0, gain_jitter=0.0, drop_prob=0.0, drop_value=0.0, axis_cnt=3, drop_thresh=None):
    def per_axis(v):
        return [float(s) for s in v] if isinstance(v, (list, tuple)) else [float(v)] * axis_cnt
    return dict(axis_cnt=axis_cnt, sigma_add=per_axis(sigma_add), sigma_mul=per_axis(sigma_mul), gain_jitter=float(gain_jitter),
                drop_thresh=int(np.floor(drop_prob * TWO24 + 0.5)) if drop_thresh is None else int(drop_thresh),
                drop_value=float(drop_value))


FULL = spec([0.02, 0.02, 0.03], [0.05, 0.05, 0.1], 0.1, 0.1, -1.5)      # every effect, per-axis sigmas
FULL2 = spec([0.02, 0.03], [0.05, 0.1], 0.1, 0.1, -1.5, axis_cnt=2)
NEUTRAL = spec()
SPECS = [
    (FULL, "every effect at once, different sigmas per axis"),
    (spec(0.02, 0.05), "noise alone: gain and dropout are skipped"),
    (spec([0.02, 0.0, 0.0], [0.0, 0.0, 0.05]), "axis 1 neutral: its elements are copied bit for bit; one sigma of each kind alone"),
    (spec(gain_jitter=0.1), "gain alone"),
    (spec(drop_prob=0.1, drop_value=-1.5), "dropout alone: the alive elements are copied bit for bit"),
]
# (C, H, W), axis_cnt: why the shape is in the table
SHAPES = [
    ((3, 4, 4), 3, "the single-frame taxels: P % 4 == 0, the 16-byte path, one gain and one dropout block per thread"),
    ((21, 4, 4), 3, "the Seqs taxels: seven frames share the gain of a taxel"),
    ((6, 4, 4), 3, "two frames"),
    ((6, 4, 4), 2, "axis_cnt 2: three frames of two axes over the same tensor"),
    ((3, 1, 1), 3, "P = 1: the scalar path, one thread covers all three channels, every element another gain block lane"),
    ((3, 5, 5), 3, "P = 25: the scalar path, threads straddle channels, 75 = 18 * 4 + 3: a ragged last thread"),
    ((3, 3, 7), 3, "P = 21, non-square: the scalar path, 63 = 15 * 4 + 3"),
]
BATCHES = (1, 7, 67, 2100)               # one thread row; several work items; more than one workgroup; several rounds of them
OFFSETS = (1, 2, 3)                      # floats off 16-byte alignment
WALKS = [(1, "one workgroup walks every item"), (3, "a stride that divides no item count: a ragged last round")]


def make_x(B, shape, seed):
    """Finite values in [-1, 1) with full mantissas."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B,) + tuple(shape), generator=g) * 2 - 1).numpy()


def make_ids(kind, B, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "none":
        return None
    if kind == "perm":
        return torch.randperm(B + 5, generator=g)[:B].numpy().astype(np.int64)
    if kind == "repeats":
        return torch.randint(0, max(1, B // 2), (B,), generator=g).numpy().astype(np.int64)
    if kind == "high":
        return (2 ** 31 - 1 - torch.randperm(B, generator=g).numpy()).astype(np.int64)
    raise ValueError(kind)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


FULL_BAR = 1e-5                          # |kernel - fp64| <= FULL_BAR max(|v|, s): eight times what plain numpy fp32 needs
F32_BAR = 2e-6                           # the bar of an fp32 restatement against fp64
GAIN_BAR = 2.0 ** -24                    # one rounding of g x


def check(got, x, sp, seed, offset, ids, id_base=0, bar=FULL_BAR):
    """The output ``got`` (B,C,H,W fp32 numpy) of the launch on ``x`` against the fp64 restatement.  Returns the worst
    |got - y| / max(|v|, s) over the elements the noise touched (0 when none).
      * a sample with an id outside [0, 2^31) is all 0x7fc00000;
      * a dead taxel holds drop_value's bits in every channel, whatever x held; the mask itself is exact (integers);
      * an alive element of a neutral axis without gain holds x's bits; with gain it is within GAIN_BAR (relative) of g x
        with g the fp32 gain of the contract -- in fact the fp32 product;
      * an alive element with noise and a finite x is finite and within ``bar`` max(|v|, s) of the fp64 value; with a
        non-finite x it is non-finite (the element's own business), and nothing else is."""
    B = x.shape[0]
    idv = np.arange(B, dtype=np.int64) + id_base if ids is None else np.asarray(ids, dtype=np.int64)
    badid = (idv < 0) | (idv >= 2 ** 31)
    r = restate(x, sp, seed, offset, np.where(badid, 0, idv))
    dead = np.broadcast_to(r["dead"].reshape(B, 1, x.shape[2], x.shape[3]), x.shape)
    okrow = np.broadcast_to(~badid.reshape(B, 1, 1, 1), x.shape)
    gb, xb = bits(got), bits(x)
    assert (gb[~okrow] == NAN_BITS).all(), "a sample with a bad id must be all-NaN"
    sel = okrow & dead
    assert (gb[sel] == bits(np.float32(sp["drop_value"]))).all(), "a dead taxel must read drop_value"
    alive = okrow & ~dead
    finite = np.isfinite(x)
    plain = alive & ~r["active"]
    if sp["gain_jitter"] == 0:
        assert (gb[plain] == xb[plain]).all(), "an untouched element must keep its bits"
    else:
        a = sp["axis_cnt"]
        P = x.shape[2] * x.shape[3]
        w = words(np.where(badid, 0, idv), (a * P + 3) // 4, 1, seed, offset)[:, :a * P].reshape(B, 1, a, P)
        g = np.broadcast_to(gain32(w, sp["gain_jitter"]), (B, x.shape[1] // a, a, P)).reshape(x.shape)
        sel = plain & finite
        with np.errstate(invalid="ignore"):
            exact = g.astype(np.float64) * x
            prod = bits(g * x)
        assert (np.abs(got[sel] - exact[sel]) <= GAIN_BAR * np.abs(exact[sel])).all(), "gain: more than one rounding of g x"
        assert (gb[sel] == prod[sel]).all(), "gain: not the fp32 product of the fp32 gain"
    noisy = alive & r["active"]
    sel = noisy & finite
    worst = 0.0
    if sel.any():
        assert np.isfinite(got[sel]).all(), "a finite element turned non-finite"
        scale = np.maximum(np.abs(r["v"][sel]), r["s"][sel])
        err = np.abs(got[sel] - r["y"][sel])
        assert (err[scale == 0] == 0).all(), "v = 0 and s = 0 (a zero under sigma_mul alone) must give 0"
        if (scale > 0).any():
            worst = float((err[scale > 0] / scale[scale > 0]).max())
        assert worst <= bar, f"worst |kernel - fp64| / max(|v|, s) = {worst:.3e} above {bar:.1e}"
    sel = alive & ~finite
    assert (~np.isfinite(got[sel])).all(), "a non-finite input element must stay non-finite"
    if sp["gain_jitter"] == 0:
        nan_in = alive & np.isnan(x) & ~r["active"]
        assert (gb[nan_in] == xb[nan_in]).all()
    return worst


# ---- statistics of a stream (limits: four sigma of the estimator; KS at the 1 % level)
def stats(n):
    """Of a flat fp64 array of would-be unit normals: (|mean| sqrt N, |var - 1| sqrt(N / 2), KS D sqrt N)."""
    n = np.sort(np.asarray(n, dtype=np.float64).ravel())
    N = n.size
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(n / np.sqrt(2.0))).numpy())
    k = np.arange(1, N + 1, dtype=np.float64)
    D = max(float((k / N - cdf).max()), float((cdf - (k - 1) / N).max()))
    return abs(float(n.mean())) * np.sqrt(N), abs(float(n.var()) - 1.0) * np.sqrt(N / 2.0), D * np.sqrt(N)


STAT_LIMITS = (4.0, 4.0, 1.63)
STAT_CASE = dict(seed=0, offset=1, B=4096, shape=(3, 4, 4))      # N = 196 608


def corr_scaled(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return abs(float(np.corrcoef(a, b)[0, 1])) * np.sqrt(a.size)


def dead_z(dead, p):
    N = dead.size
    return abs(float(dead.sum()) - N * p) / np.sqrt(N * p * (1 - p))


# ---- refusals: (label, overrides of BASE_ARGS); pointers: 1 = given (a small fake address), 0 = NULL
BASE_ARGS = dict(x=1, out=1, B=4, C=3, H=4, W=4, axis_cnt=3, sigma_add=[0.02] * 3, sigma_mul=[0.05] * 3, gain_jitter=0.1,
                 drop_thresh=1000, drop_value=0.0, ids=0, id_base=0, seed=1, offset=1)
INF, NANF = float("inf"), float("nan")
REFUSALS = [
    ("null x", dict(x=0)), ("null out", dict(out=0)),
    ("B 0", dict(B=0)), ("B -1", dict(B=-1)), ("C 0", dict(C=0)), ("C -3", dict(C=-3)), ("H 0", dict(H=0)), ("H -4", dict(H=-4)),
    ("W 0", dict(W=0)), ("W -4", dict(W=-4)),
    ("axis_cnt 0", dict(axis_cnt=0)), ("axis_cnt 5", dict(axis_cnt=5, C=5, sigma_add=[0.0] * 5, sigma_mul=[0.0] * 5)),
    ("axis_cnt -1", dict(axis_cnt=-1)), ("C % axis_cnt", dict(C=4)), ("C % axis_cnt, axis_cnt 2", dict(axis_cnt=2)),
    ("C*H*W = 2^31", dict(C=2 << 10, H=1 << 10, W=1 << 10, axis_cnt=2, sigma_add=[0.02] * 2, sigma_mul=[0.05] * 2)),
    ("C*H*W = 3 * 2^30", dict(C=3 << 10, H=1 << 10, W=1 << 10)),
    ("C*H*W wraps 32 bits", dict(C=3 << 14, H=1 << 16, W=1 << 16)),
    ("sigma_add negative", dict(sigma_add=[0.02, -0.01, 0.02])), ("sigma_mul negative", dict(sigma_mul=[-1.0, 0.0, 0.0])),
    ("sigma_add NaN", dict(sigma_add=[0.02, 0.02, NANF])), ("sigma_mul NaN", dict(sigma_mul=[NANF, 0.0, 0.0])),
    ("sigma_add Inf", dict(sigma_add=[INF, 0.0, 0.0])), ("sigma_mul Inf", dict(sigma_mul=[0.0, INF, 0.0])),
    ("gain_jitter NaN", dict(gain_jitter=NANF)), ("gain_jitter Inf", dict(gain_jitter=INF)),
    ("drop_value NaN", dict(drop_value=NANF)), ("drop_value -Inf", dict(drop_value=-INF)),
    ("drop_thresh -1", dict(drop_thresh=-1)), ("drop_thresh 2^24 + 1", dict(drop_thresh=TWO24 + 1)),
    ("partial overlap, out ahead", dict(overlap=4)), ("partial overlap, out behind", dict(overlap=-16)),
    ("partial overlap by the last float", dict(overlap=4 * (4 * 48 - 1))),
    ("max_wgs 0", dict(max_wgs=0)), ("max_wgs -1", dict(max_wgs=-1)), ("null x through _wgs", dict(max_wgs=4, x=0)),
    ("null rng", dict(rng=0)), ("null out through _dev", dict(rng=1, out=0)), ("drop_thresh through _dev", dict(rng=1, drop_thresh=-5)),
]
BITS_BASE = dict(out=1, B=2, blocks=3, ids=0, id_base=0, tag=0, seed=0, offset=0)
BITS_REFUSALS = [("null out", dict(out=0)), ("B 0", dict(B=0)), ("B -2", dict(B=-2)), ("blocks 0", dict(blocks=0)),
                 ("blocks -1", dict(blocks=-1)), ("tag -1", dict(tag=-1))]
ADDR = dict(x=1 << 20, out=1 << 21, ids=1 << 22, rng=1 << 23)


def call_raw(lib, a, stream=0, **ptrs):
    """tsr_taxel_noise with the scalars of ``a``; tsr_taxel_noise_wgs when ``a`` holds ``max_wgs``, tsr_taxel_noise_dev when
    it holds ``rng``.  A pointer is ``ptrs[name]`` when given, else the fake address ADDR[name] nothing may dereference
    (a[name] = 1) or NULL (a[name] = 0); ``overlap`` = d puts out d bytes after x.  Returns the status."""
    P = ctypes.c_void_p

    def p(name):
        return ptrs[name] if name in ptrs else (ADDR[name] if a.get(name) else 0)
    xa, oa = p("x"), p("out")
    if "overlap" in a:
        oa = xa + a["overlap"]
    n = max(len(a["sigma_add"]), 1)
    sa = (ctypes.c_float * n)(*a["sigma_add"])
    sm = (ctypes.c_float * n)(*a["sigma_mul"])
    head = (P(xa), P(oa), a["B"], a["C"], a["H"], a["W"], a["axis_cnt"], ctypes.cast(sa, P), ctypes.cast(sm, P),
            ctypes.c_float(a["gain_jitter"]), a["drop_thresh"], ctypes.c_float(a["drop_value"]), P(p("ids")), a["id_base"])
    if "rng" in a:
        return lib.tsr_taxel_noise_dev(*head, P(p("rng")), P(stream))
    tail = (ctypes.c_ulonglong(a["seed"]), ctypes.c_uint(a["offset"]))
    if "max_wgs" in a:
        return lib.tsr_taxel_noise_wgs(*head, *tail, a["max_wgs"], P(stream))
    return lib.tsr_taxel_noise(*head, *tail, P(stream))


def call_bits_raw(lib, a, stream=0, **ptrs):
    P = ctypes.c_void_p

    def p(name):
        return ptrs[name] if name in ptrs else (ADDR[name] if a.get(name) else 0)
    return lib.tsr_taxel_noise_bits(P(p("out")), a["B"], a["blocks"], P(p("ids")), a["id_base"], a["tag"],
                                    ctypes.c_ulonglong(a["seed"]), ctypes.c_uint(a["offset"]), P(stream))


# ---- the guarded launch (ROCm tensors)
def placed(n, off, guard, fill=None):
    """n floats starting ``off`` floats past a 16-byte boundary inside a NaN-filled device buffer with at least ``guard`` NaN
    floats on either side: (buffer, the view, its start)."""
    start = (guard + 3) // 4 * 4 + off
    buf = torch.full((start + n + guard + 4,), float("nan"), dtype=torch.float32, device="cuda")
    mid = buf[start:start + n]
    assert mid.data_ptr() % 16 == 4 * off
    if fill is not None:
        mid.copy_(torch.as_tensor(fill).reshape(-1))
    return buf, mid, start


def launch(lib, x, sp, seed=0, offset=0, ids=None, id_base=0, x_off=0, out_off=0, inplace=False, max_wgs=None, rng=None,
           expect=0):
    """One raw launch of ``x`` (B,C,H,W fp32 numpy), twice into fresh buffers: the output as numpy.  The output is prefilled
    with NaN (out of place) and sits between NaN guard bands that must stay NaN; x sits in a guarded buffer of its own and
    must come back unchanged (out of place).  ``rng`` = (seed, offset) takes the _dev form with the words on the device."""
    B, C, H, W = x.shape
    n = x.size
    guard = max(C * H * W, 64)
    idd = None if ids is None else torch.as_tensor(np.asarray(ids, dtype=np.int64)).cuda()
    a = dict(B=B, C=C, H=H, W=W, axis_cnt=sp["axis_cnt"], sigma_add=sp["sigma_add"], sigma_mul=sp["sigma_mul"],
             gain_jitter=sp["gain_jitter"], drop_thresh=sp["drop_thresh"], drop_value=sp["drop_value"], id_base=id_base,
             seed=seed, offset=offset)
    if max_wgs is not None:
        a["max_wgs"] = max_wgs
    rd = None
    if rng is not None:
        s = int(rng[0]) % (1 << 64)
        rd = torch.from_numpy(np.array([s & 0xffffffff, s >> 32, rng[1], 0], dtype=np.uint32).view(np.int32)).cuda()
        a["rng"] = 1
    outs = []
    for _ in range(2):
        xbuf, xd, xs = placed(n, x_off, guard, torch.from_numpy(x))
        if inplace:
            obuf, od, os_ = xbuf, xd, xs
        else:
            obuf, od, os_ = placed(n, out_off, guard)
        st = call_raw(lib, a, stream=torch.cuda.current_stream().cuda_stream, x=xd.data_ptr(), out=od.data_ptr(),
                      ids=0 if idd is None else idd.data_ptr(), rng=0 if rd is None else rd.data_ptr())
        assert st == expect, st
        torch.cuda.synchronize()
        assert bool(torch.isnan(obuf[:os_]).all() and torch.isnan(obuf[os_ + n:]).all()), "guard band written"
        if not inplace:
            assert_same_bits(xd.cpu().numpy().reshape(x.shape), x, "x was written")
        outs.append(od.cpu().numpy().reshape(x.shape).copy())
    assert_same_bits(outs[0], outs[1], "two launches")
    return outs[0]
