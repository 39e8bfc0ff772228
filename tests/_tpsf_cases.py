"""Yardstick, comparison rule, case tables and input builders of tests/test_gpu_tpsf_kernels.py (tpsf_forward / tpsf_backward,
csrc/tpsf_mfma.hip, and the refusals / empty splits of the tsr_sgemm family, csrc/sgemm_mfma.hip).  Nothing here touches a
device: tests/test_tpsf_cases_cpu.py checks every precondition the GPU tests rely on.

The yardstick is the operation itself in fp64 matrix form, differentiable by autograd (reference model/tPSFNet.py:78-141):

    HR  = alpha * G D G,   G[i][j] = exp(-(100/4802) (i-j)^2 / beta^2) for |i-j| <= 49, else 0
    plateau = D > D.max() - 1e-3, filled with the detached max(HR off the plateau, 0)
    LR[a][c] = (E_a . HR . E_c - mn * sum HR) / (1 - mn) * 1e-4,  E_a[x] = exp(-(100/15138) (x - (12 + 25 a))^2 / gamma),
               mn = exp(-100 / gamma)
    psf[u][v] = alpha * g(u - 49) g(v - 49)

It agrees with the oracle's direct 99x99 convolution in fp64 to 1e-7 (the oracle keeps its fp32 geometry tables) and costs
milliseconds per sample instead of half a second.

THE RULE for every comparison against it:   |kernel - fp64| <= max(1e-5 * scale, 4 * |fp32 reference - fp64|)  per element,
where the fp32 reference is the oracle's tpsf_forward_from_ab in float32 with autograd and `scale` is stated per check: the
project's tPSFNet bar of 1e-5 on the quantity's OWN scale, and -- for the ill-conditioned quantities (signed sums) -- four times
what the reference formula itself loses in fp32 (the two significand bits the kernel's two fp16 planes, 22 bits, lack against
fp32's 24).  The second term is capped: for every case it stays below 1e-3 of the scale (CPU test), so no element goes unchecked.
"""
import ctypes
import functools
from collections import namedtuple

import torch

KP = 100.0 / 4802.0
KM = 100.0 / 15138.0
BAR = 1e-5                 # the project's tPSFNet bar
FP32_FACTOR = 4.0          # two significand bits
FP32_CAP = 1e-3            # the fp32-reference term never exceeds this fraction of the scale
MAX_FP32_SAMPLES = 12      # the direct convolution is slow: at most this many samples per test get the fp32 term
NAN = float("nan")

Case = namedtuple("Case", "name depth ab dl fp32_idx")      # depth (B,100,100), ab (B,3), dl (B,16) fp32; fp32_idx: samples
Ref = namedtuple("Ref", "HR LR psf dab")                   # (n,100,100), (n,16), (n,99,99), (n,3) fp64


# ----------------------------------------------------------------------------------------------------------- the yardstick
def gauss_tap(beta, d):
    """g(d) = exp(-(100/4802) d^2 / beta^2) in fp64."""
    return torch.exp(-KP * torch.as_tensor(d, dtype=torch.float64) ** 2 / torch.as_tensor(beta, dtype=torch.float64) ** 2)


def forward64(ab, depth):
    """(HR (B,100,100), LR_deg (B,16), psf (B,99,99)) in fp64 from ab (B,3) fp64 (may require grad) and depth (B,100,100)."""
    assert ab.dtype == torch.float64 and depth.dtype == torch.float64
    alpha, beta, gamma = (ab[:, j].view(-1, 1, 1) for j in range(3))
    i = torch.arange(100, dtype=torch.float64)
    d = (i.view(-1, 1) - i.view(1, -1)).unsqueeze(0)
    G = torch.where(d.abs() <= 49, torch.exp(-KP * d * d / (beta * beta)), torch.zeros((), dtype=torch.float64))
    HR = alpha * (G @ depth @ G)
    mask = depth > depth.amax(dim=(1, 2), keepdim=True) - 1e-3
    fill = HR.detach().masked_fill(mask, 0.0).amax(dim=(1, 2), keepdim=True)     # the mask is never empty: 0 takes part
    HR = torch.where(mask, fill, HR)
    c = (12 + 25 * torch.arange(4, dtype=torch.float64)).view(1, 4, 1)
    E = torch.exp(-KM * (i.view(1, 1, -1) - c) ** 2 / gamma)                     # (B,4,100)
    mn = torch.exp(-100.0 / gamma)
    LR = (E @ HR @ E.transpose(1, 2) - mn * HR.sum(dim=(1, 2), keepdim=True)) / (1 - mn) * 1e-4
    u = torch.arange(99, dtype=torch.float64) - 49
    g = torch.exp(-KP * u.view(1, -1) ** 2 / (beta.view(-1, 1) ** 2))
    psf = alpha * g.unsqueeze(2) * g.unsqueeze(1)
    return HR, LR.reshape(-1, 16), psf


def reference64(case, idx=None):
    """fp64 outputs and d(sum LR_deg * dl)/d(alpha, beta, gamma) of the samples `idx` (all by default)."""
    idx = torch.arange(case.depth.shape[0]) if idx is None else torch.as_tensor(idx)
    ab = case.ab[idx].double().requires_grad_(True)
    HR, LR, psf = forward64(ab, case.depth[idx].double())
    (LR * case.dl[idx].double()).sum().backward()
    return Ref(HR.detach(), LR.detach(), psf.detach(), ab.grad.detach())


def oracle_reference(case, idx, dtype):
    """The same four quantities from the oracle's direct convolution in `dtype` (fp32: the second term of the rule)."""
    from oracle import tactilesr_oracle as O
    idx = torch.as_tensor(idx)
    n = len(idx)
    ab = case.ab[idx].to(dtype).requires_grad_(True)
    HR, LR, psf = O.tpsf_forward_from_ab(ab, case.depth[idx].to(dtype))
    (LR.reshape(n, 16) * case.dl[idx].to(dtype)).sum().backward()
    return Ref(HR.detach().view(n, 100, 100).double(), LR.detach().view(n, 16).double(), psf.detach().view(n, 99, 99).double(),
               ab.grad.detach().double())


@functools.lru_cache(maxsize=None)
def fp32_reference(name):
    """Oracle in float32 on the case's fp32_idx samples, computed once per process and never modified."""
    case = CASES[name]()
    assert len(case.fp32_idx) <= MAX_FP32_SAMPLES
    return oracle_reference(case, case.fp32_idx, torch.float32)


# ------------------------------------------------------------------------------------------------------------------ the rule
def sample_scale(ref):
    """max |ref| of every sample, broadcastable against ref."""
    return ref.abs().flatten(1).amax(dim=1).view(-1, *([1] * (ref.dim() - 1)))


def rule_bar(ref64, scale, ref32=None, rows32=None):
    """Per-element bar of the rule.  ref32 (optional) holds the fp32 reference of the rows `rows32` of ref64 (all rows when
    None); the other rows get the plain 1e-5 * scale."""
    bar = (BAR * scale).expand_as(ref64).clone()
    if ref32 is not None:
        rows = torch.arange(ref64.shape[0]) if rows32 is None else torch.as_tensor(rows32)
        bar[rows] = torch.maximum(bar[rows], FP32_FACTOR * (ref32 - ref64[rows]).abs())
    return bar


def check(label, got, ref64, scale, ref32=None, rows32=None):
    """Assert the rule element by element; print the kernel's worst error and the fp32 reference's worst error on the rows that
    have one, both as fractions of the scale."""
    got = got.detach().cpu().double()
    scale = torch.as_tensor(scale, dtype=torch.float64)
    err = (got - ref64).abs()
    bar = rule_bar(ref64, scale, ref32, rows32)
    den = scale.expand_as(ref64).clamp_min(1e-300)
    worst = float((err / den).max())
    if ref32 is not None:
        rows = torch.arange(ref64.shape[0]) if rows32 is None else torch.as_tensor(rows32)
        w32 = float(((ref32 - ref64[rows]).abs() / den[rows]).max())
        wk = float((err[rows] / den[rows]).max())
        print(f"[tpsf kernels] {label}: kernel {worst:.1e} (on the fp32-reference rows {wk:.1e}), fp32 reference {w32:.1e}")
    else:
        print(f"[tpsf kernels] {label}: kernel {worst:.1e} (closed form, no fp32 reference)")
    bad = ~(err <= bar)                               # NaN fails
    assert not bool(bad.any()), (label, int(bad.sum()), worst, bad.nonzero()[:5].tolist())
    return worst


def plateau_margin(depth, skip_max=False):
    """Smallest distance of a pixel from depth.max() - 1e-3, as a fraction of max(|depth|, 1e-3), over the batch: above 2e-7
    the fp32 kernel and the fp64 yardstick agree on the plateau (the fp32 threshold is off by at most half an ulp of the
    maximum, 6e-8).  skip_max leaves out the pixels that equal the maximum: they are always exactly 1e-3 above the threshold,
    which is less than 2e-7 of a maximum above 5000 (the impulse of 2e4); for them see max_pixel_is_on_the_fp32_plateau."""
    d = depth.double()
    top = d.amax(dim=(1, 2), keepdim=True)
    mx = d.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-3)
    m = (d - (top - 1e-3)).abs() / mx
    if skip_max:
        m = m.masked_fill(d == top, float("inf"))
    return float(m.min())


def max_pixel_is_on_the_fp32_plateau(depth):
    """depth.max() > depth.max() - 1e-3 evaluated in fp32 as the kernel (and the reference model) evaluates it: true while the
    fp32 subtraction still moves the maximum, i.e. for maxima below 2^15."""
    top = depth.float().amax(dim=(1, 2))
    return bool((top > top - torch.tensor(1e-3, dtype=torch.float32)).all())


# --------------------------------------------------------------------------------------------------------------- case tables
def draw_ab(n, g):
    """(alpha, beta, gamma) as test_tpsf_kernels_wide_dynamic_range_batch draws them."""
    return torch.rand(n, 3, generator=g) * torch.tensor([1.0, 3.0, 2.0]) + torch.tensor([0.2, 0.25, 0.6])


def positive_dl(n, g):
    return torch.randn(n, 16, generator=g).abs() + 0.1


# 1. impulses.  Positions: corners; wave seams (rows 31|32, 63|64, 95|96); last wave rows 96..99 and column tile 3 (x = 96..99);
# the two pixels whose +-49 band ends exactly at the image edge.  v cycles 1, 3e-3, 2e4 in table order, which gives every
# diagonal position v = 1.
IMPULSE_WIDE = (0.7, 10.0, 1.3)
IMPULSE_NARROW = (0.7, 0.05, 1.3)
IMPULSE_VALUES = (1.0, 3e-3, 2e4)
IMPULSE_POSITIONS = [(0, 0), (0, 99), (99, 0), (99, 99),
                     (31, 50), (32, 50), (63, 64), (64, 63), (95, 10), (96, 10),
                     (99, 96), (96, 99), (97, 97), (50, 95), (50, 96), (10, 99),
                     (49, 50), (50, 49)]
IMPULSE_NARROW_POSITIONS = [(63, 64), (96, 99)]
IMPULSE_BACKWARD_POSITIONS = [(40, 60), (97, 3), (64, 96)]          # wide; gradients compared
IMPULSE_ALL = IMPULSE_POSITIONS + IMPULSE_NARROW_POSITIONS + IMPULSE_BACKWARD_POSITIONS
IMPULSE_BACKWARD = [20, 21, 22]
IMPULSE_FP32 = [0, 3, 5, 9, 10, 12, 16, 18, 19] + IMPULSE_BACKWARD


def impulse_value(i):
    return IMPULSE_VALUES[i % 3]


def impulse_params(i):
    n = len(IMPULSE_POSITIONS)
    return IMPULSE_NARROW if n <= i < n + len(IMPULSE_NARROW_POSITIONS) else IMPULSE_WIDE


def impulse_case():
    B = len(IMPULSE_ALL)
    depth = torch.zeros(B, 100, 100)
    for i, (y, x) in enumerate(IMPULSE_ALL):
        depth[i, y, x] = impulse_value(i)
    ab = torch.tensor([impulse_params(i) for i in range(B)])
    return Case("impulse", depth, ab, positive_dl(B, torch.Generator().manual_seed(21)), IMPULSE_FP32)


def impulse_closed_form(i):
    """alpha * v * g(y - y0) g(x - x0) off the impulse pixel, exactly 0 beyond +-49; the pixel itself (the plateau) holds the
    largest of the others.  fp64; the value, alpha and beta are taken as the fp32 numbers the kernel receives."""
    y0, x0 = IMPULSE_ALL[i]
    a, b, _ = (float(torch.tensor(t, dtype=torch.float32)) for t in impulse_params(i))
    v = float(torch.tensor(impulse_value(i), dtype=torch.float32))
    k = torch.arange(100, dtype=torch.float64)
    gy = torch.where((k - y0).abs() <= 49, gauss_tap(b, k - y0), torch.zeros((), dtype=torch.float64))
    gx = torch.where((k - x0).abs() <= 49, gauss_tap(b, k - x0), torch.zeros((), dtype=torch.float64))
    HR = a * v * gy.view(-1, 1) * gx.view(1, -1)
    HR[y0, x0] = 0.0
    HR[y0, x0] = HR.max()
    return HR


def psf_closed_form(ab):
    """alpha g(u) g(v) in fp64 from the fp32 rows of ab (B,3)."""
    ab = ab.double()
    u = torch.arange(99, dtype=torch.float64) - 49
    g = gauss_tap(ab[:, 1].view(-1, 1), u.view(1, -1))
    return ab[:, 0].view(-1, 1, 1) * g.unsqueeze(2) * g.unsqueeze(1)


# 2. conditioned inputs: positive depth over six decades, positive dLR_deg -- d/dalpha and d/dbeta are sums of like-signed terms
def conditioned_case():
    g = torch.Generator().manual_seed(31)
    depth = torch.rand(12, 100, 100, generator=g) * 10
    depth = depth * torch.pow(10.0, (torch.arange(12) % 6 - 3).double()).float().view(12, 1, 1)
    ab = draw_ab(12, g)
    return Case("conditioned", depth, ab, positive_dl(12, g), list(range(12)))


# 3. the first 12 samples of test_tpsf_kernels_wide_dynamic_range_batch (tests/test_gpu_tpsf.py), drawn exactly as it draws them
def signed_case():
    B = 300
    g = torch.Generator().manual_seed(5)
    depth = torch.rand(B, 100, 100, generator=g) * 10
    depth[1] = depth[1] * 1e-3
    depth[2] = (depth[2] - 5) * 40
    depth[3] = 0
    depth[3, 40:60, 40:60] = 7.5
    ab = torch.rand(B, 3, generator=g) * torch.tensor([1.0, 3.0, 2.0]) + torch.tensor([0.2, 0.25, 0.6])
    dl = torch.randn(B, 16, generator=g)
    return Case("signed", depth[:12].clone(), ab[:12].clone(), dl[:12].clone(), list(range(12)))


# 4. degenerate plateaus
DEGENERATE = ["constant", "zeros", "spike", "negative", "levels", "block_tile3", "block_lastwave"]
SPIKE_AT, SPIKE_VALUE = (37, 58), -5.0
LEVEL_MAX = 2.0


def degenerate_case():
    g = torch.Generator().manual_seed(41)
    n = len(DEGENERATE)
    depth = torch.zeros(n, 100, 100)
    depth[0] = 3.0
    depth[2, SPIKE_AT[0], SPIKE_AT[1]] = SPIKE_VALUE
    depth[3] = -(torch.rand(100, 100, generator=g) * 10 + 0.5)
    lv = torch.randint(0, 3, (100, 100), generator=g)
    depth[4] = torch.tensor([LEVEL_MAX, LEVEL_MAX - 5e-4, LEVEL_MAX - 2e-3])[lv]
    depth[5] = torch.rand(100, 100, generator=g) * 5
    depth[5, 30:35, 94:100] = 7.5
    depth[6] = torch.rand(100, 100, generator=g) * 5
    depth[6, 95:100, 0:41] = 7.5
    return Case("degenerate", depth, draw_ab(n, g), positive_dl(n, g), list(range(n)))


# 5. parameter corners: the product of the ends, on a positive and on a signed depth
CORNER_ALPHA, CORNER_BETA, CORNER_GAMMA = (1e-3, 50.0), (0.03, 30.0), (0.05, 50.0)
CORNERS = [(a, b, c) for a in CORNER_ALPHA for b in CORNER_BETA for c in CORNER_GAMMA]


def _corner_case(signed):
    g = torch.Generator().manual_seed(51 + signed)
    d = torch.rand(100, 100, generator=g) * 10
    if signed:
        d = (d - 5) * 4
    n = len(CORNERS)
    return Case("corners_signed" if signed else "corners_positive", d.unsqueeze(0).repeat(n, 1, 1), torch.tensor(CORNERS),
                positive_dl(n, g), list(range(n)))


def corners_positive_case():
    return _corner_case(0)


def corners_signed_case():
    return _corner_case(1)


CASES = {"impulse": impulse_case, "conditioned": conditioned_case, "signed": signed_case, "degenerate": degenerate_case,
         "corners_positive": corners_positive_case, "corners_signed": corners_signed_case}

# 6. isolation: B = 600 -> forward workgroups 0..87 (grid 512) take a second sample, every tpsf_bwd_dhb workgroup (grid 256) a
# second or third; samples 0..15 are poisoned in the second run, so the samples that FOLLOW them in a workgroup (512..527 in the
# forward; 256.., 512.. in tpsf_bwd_dhb) are among the compared ones
ISOLATION_B = 600
ISOLATION_POISONED = 16
FWD_GRID, DHB_GRID = 512, 256


def isolation_inputs(poisoned):
    g = torch.Generator().manual_seed(61)
    B = ISOLATION_B
    depth = torch.rand(B, 100, 100, generator=g) * 10
    depth = depth * torch.pow(10.0, (torch.arange(B) % 5 - 2).double()).float().view(B, 1, 1)
    ab = draw_ab(B, g)
    dl = torch.randn(B, 16, generator=g)
    if poisoned:
        for b in range(8):                                 # a NaN or +Inf pixel, on the seams as well
            y, x = [(0, 0), (31, 50), (96, 96), (99, 99), (50, 49), (64, 95), (10, 99), (97, 3)][b]
            depth[b, y, x] = NAN if b % 2 == 0 else float("inf")
        for b in range(8, 16):
            ab[b, (b - 8) % 3] = NAN
    return depth, ab, dl


# ------------------------------------------------------------------------------------------------------ 7. refusals, 8. splits
SG_KT = 32                 # K step of sgemm_tile_kernel: split ranges are whole K steps
EMPTY_SPLIT_SHAPES = [(5, 70, 3, 4), (130, 3, 17, 8), (3, 256, 40, 32)]       # (M, N, K, nsplit)
EMPTY_COLSUM = (3, 70, 5)                                                     # (M rows, N, nsplit)


def splitk_chunk(K, nsplit):
    """K range of one split: ceil(K / nsplit) rounded up to whole K steps (include/tactilesr_hip.h)."""
    return -(-(-(-K // nsplit)) // SG_KT) * SG_KT


def nonempty_splits(K, nsplit):
    return min(nsplit, -(-K // splitk_chunk(K, nsplit)))


REFUSAL_TPSF_B = 2
REFUSAL_MNK = (8, 8, 8)


def refusal_table(p):
    """[(label, entry point, ctypes argument list)]: every call must return 1 before any HIP call.  p(name) -> c_void_p of the
    buffer `name`; the stream is NULL (never used)."""
    I, L, N0 = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p(0)
    M, N, K = REFUSAL_MNK
    B = REFUSAL_TPSF_B
    rows = []
    fwd = ["depth", "ab", "HR", "LRd", "psf"]
    bwd = ["depth", "ab", "HR", "dl", "dab", "work"]
    for names, fn in ((fwd, "tpsf_forward"), (bwd, "tpsf_backward")):
        for k in range(len(names)):
            rows.append((f"{fn} NULL {names[k]}", fn, [N0 if j == k else p(n) for j, n in enumerate(names)] + [I(B), N0]))
        for bad in (0, -1):
            rows.append((f"{fn} B={bad}", fn, [p(n) for n in names] + [I(bad), N0]))

    def sgemm(A="A", Bm="Bm", C="C", m=M, n=N, k=K, act=0):
        return [p(A) if A else N0, L(K), L(1), p(Bm) if Bm else N0, L(N), L(1), p("bias"), p(C) if C else N0, I(m), I(n), I(k),
                I(act), N0]
    rows += [("tsr_sgemm NULL A", "tsr_sgemm", sgemm(A=None)), ("tsr_sgemm NULL B", "tsr_sgemm", sgemm(Bm=None)),
             ("tsr_sgemm NULL C", "tsr_sgemm", sgemm(C=None))]
    for bad in (0, -1):
        rows += [(f"tsr_sgemm M={bad}", "tsr_sgemm", sgemm(m=bad)), (f"tsr_sgemm N={bad}", "tsr_sgemm", sgemm(n=bad)),
                 (f"tsr_sgemm K={bad}", "tsr_sgemm", sgemm(k=bad))]
    rows += [("tsr_sgemm act=-1", "tsr_sgemm", sgemm(act=-1)), ("tsr_sgemm act=3", "tsr_sgemm", sgemm(act=3))]
    ab_ = [p("A"), L(K), L(1), p("Bm"), L(N), L(1)]
    rows.append(("tsr_sgemm_masked NULL mask", "tsr_sgemm_masked", ab_ + [N0, p("C"), I(M), I(N), I(K), N0]))
    for ns in (0, 65536):
        rows.append((f"tsr_sgemm_splitk nsplit={ns}", "tsr_sgemm_splitk", ab_ + [p("slab"), I(M), I(N), I(K), I(ns), N0]))
        rows.append((f"tsr_sgemm_splitk_strided nsplit={ns}", "tsr_sgemm_splitk_strided",
                     ab_ + [p("slab"), L(M * N), I(M), I(N), I(K), I(ns), N0]))
    rows.append(("tsr_sgemm_splitk_strided split_stride=M*N-1", "tsr_sgemm_splitk_strided",
                 ab_ + [p("slab"), L(M * N - 1), I(M), I(N), I(K), I(2), N0]))
    rows.append(("tsr_colsum_splitk split_stride=N-1", "tsr_colsum_splitk", [p("C"), p("slab"), L(N - 1), I(M), I(N), I(2), N0]))
    return rows
