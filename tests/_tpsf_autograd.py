"""Upstream gradients, scenario tables, references and input builders of tests/test_gpu_tpsf_autograd.py (tpsf_backward_ex and
the autograd of tactilesr_amd.tPSFNet).  Nothing here touches a device: tests/test_tpsf_autograd_cpu.py checks every precondition
the GPU tests rely on.  Yardstick (forward64), rule (check / rule_bar), depth / (alpha, beta, gamma) / dLR_deg tables: _tpsf_cases.

A SCENARIO is (case of _tpsf_cases, upstream kind, mode):
    kind  "positive"  dHR = rand + 0.1, dpsf = rand + 0.1 (every sum is a sum of like-signed terms where the case's own is)
          "signed"    dHR = randn, dpsf = randn
    mode  "hr"   dHR alone (dLR_deg NULL)        "psf"  dpsf alone        "all"  dLR_deg (the case's own) + dHR + dpsf
dHR is scaled by 1e-4, the factor LR_deg carries, so that in mode "all" both terms of the per-pixel weight matter.

References: torch.autograd.grad of  sum HR*dHR + sum LR*dLR + sum psf*dpsf  w.r.t. (ab, depth) through forward64 in fp64, and
through the oracle's tpsf_forward_from_ab in float32 (the second term of the rule) on FP32_ROWS samples of the case -- the direct
99x99 convolution's backward costs a quarter of a second per sample and scenario, so three samples per case carry it; every other
row is held to the plain 1e-5 of its scale.
"""
import ctypes
import functools
from collections import namedtuple

import torch

import _tpsf_cases as T

KINDS = ("positive", "signed")
MODES = ("hr", "psf", "all")
AG_CASES = ("conditioned", "signed", "degenerate", "corners_positive", "corners_signed")
# samples that carry the fp32-oracle term: the signed-large and block-plateau samples of "signed", the two block plateaus and the
# three-level depth of "degenerate", a narrow and two wide corners
FP32_ROWS = {"conditioned": [0, 5, 10], "signed": [1, 2, 3], "degenerate": [4, 5, 6], "corners_positive": [0, 3, 6],
             "corners_signed": [1, 2, 7]}
HR_UP_SCALE = 1e-4

Up = namedtuple("Up", "dl dHR dpsf")                 # (B,16), (B,100,100), (B,99,99) fp32, or None
Grads = namedtuple("Grads", "dab dd")                # (n,3), (n,100,100) fp64


def upstream(name, kind):
    """dHR (B,100,100) and dpsf (B,99,99) of the case `name`, fp32, seeded by (name, kind)."""
    B = T.CASES[name]().depth.shape[0]
    g = torch.Generator().manual_seed(7000 + 10 * AG_CASES.index(name) + KINDS.index(kind))
    if kind == "positive":
        return (torch.rand(B, 100, 100, generator=g) + 0.1) * HR_UP_SCALE, torch.rand(B, 99, 99, generator=g) + 0.1
    return torch.randn(B, 100, 100, generator=g) * HR_UP_SCALE, torch.randn(B, 99, 99, generator=g)


def scenario_up(name, kind, mode):
    case = T.CASES[name]()
    dHR, dpsf = upstream(name, kind)
    return Up(case.dl if mode == "all" else None, dHR if mode in ("hr", "all") else None, dpsf if mode in ("psf", "all") else None)


def loss_of(HR, LR, psf, up, dtype):
    n = HR.shape[0]
    loss = 0
    if up.dHR is not None:
        loss = loss + (HR.reshape(n, 100, 100) * up.dHR.to(dtype)).sum()
    if up.dl is not None:
        loss = loss + (LR.reshape(n, 16) * up.dl.to(dtype)).sum()
    if up.dpsf is not None:
        loss = loss + (psf.reshape(n, 99, 99) * up.dpsf.to(dtype)).sum()
    return loss


def take(up, idx):
    return Up(*(None if t is None else t[idx] for t in up))


def grads64(depth, ab, up, idx=None):
    """d loss / d (ab, depth) of the samples `idx` through forward64: the yardstick."""
    idx = torch.arange(depth.shape[0]) if idx is None else torch.as_tensor(idx)
    a = ab[idx].double().requires_grad_(True)
    d = depth[idx].double().requires_grad_(True)
    HR, LR, psf = T.forward64(a, d)
    dab, dd = torch.autograd.grad(loss_of(HR, LR, psf, take(up, idx), torch.float64), (a, d), allow_unused=True)
    dd = torch.zeros_like(d) if dd is None else dd          # dpsf alone: nothing reaches the depth
    return Grads(dab.detach(), dd.detach())


@functools.lru_cache(maxsize=None)
def fp32_grads(name):
    """{(kind, mode): Grads} of the oracle in float32 on FP32_ROWS[name]: ONE forward, one backward per scenario; computed once
    per process and never modified."""
    from oracle import tactilesr_oracle as O
    case = T.CASES[name]()
    idx = torch.tensor(FP32_ROWS[name])
    assert len(idx) <= T.MAX_FP32_SAMPLES
    a = case.ab[idx].clone().requires_grad_(True)
    d = case.depth[idx].clone().requires_grad_(True)
    HR, LR, psf = O.tpsf_forward_from_ab(a, d)
    out = {}
    for kind in KINDS:
        for mode in MODES:
            up = take(scenario_up(name, kind, mode), idx)
            dab, dd = torch.autograd.grad(loss_of(HR, LR, psf, up, torch.float32), (a, d), retain_graph=True, allow_unused=True)
            dd = torch.zeros_like(d) if dd is None else dd
            out[(kind, mode)] = Grads(dab.detach().double(), dd.detach().double())
    return out


def dab_scale(name, kind, ref_dab):
    """The scale of a d(alpha, beta, gamma) check: the component itself where every sum is like-signed (the conditioned case
    under positive upstream gradients), else the sample's largest component."""
    if name == "conditioned" and kind == "positive":
        return ref_dab.abs()
    return ref_dab.abs().amax(dim=1, keepdim=True)


# ------------------------------------------------------------------------------------------------- the closed forms (the issue)
def closed_form(depth, ab, up):
    """d(alpha, beta, gamma) (B,3; gamma only when no dLR_deg is given, else NaN there) and d_depth (B,100,100) in fp64 from the
    formulas include/tactilesr_hip.h documents, written out per sample with explicit matrices."""
    B = depth.shape[0]
    k = torch.arange(100, dtype=torch.float64)
    D = k.view(-1, 1) - k.view(1, -1)
    u = torch.arange(99, dtype=torch.float64) - 49
    cx = 12 + 25 * torch.arange(4, dtype=torch.float64)
    dab = torch.zeros(B, 3, dtype=torch.float64)
    dd = torch.zeros(B, 100, 100, dtype=torch.float64)
    for b in range(B):
        al, be, ga = (float(v) for v in ab[b].double())
        d = depth[b].double()
        G = torch.where(D.abs() <= 49, torch.exp(-T.KP * D * D / be ** 2), torch.zeros((), dtype=torch.float64))
        H = D * D * G
        P = d > d.max() - 1e-3
        W = torch.zeros(100, 100, dtype=torch.float64)
        if up.dHR is not None:
            W = W + up.dHR[b].double()
        if up.dl is not None:
            E = torch.exp(-T.KM * (k.view(1, -1) - cx.view(-1, 1)) ** 2 / ga)             # (4,100)
            mn = torch.exp(torch.tensor(-100.0 / ga, dtype=torch.float64))
            m = (E.view(4, 1, 100, 1) * E.view(1, 4, 1, 100) - mn) / (1 - mn)             # m_ac[y][x]
            W = W + 1e-4 * (up.dl[b].double().view(4, 4, 1, 1) * m).sum((0, 1))
            dab[b, 2] = float("nan")
        W = W.masked_fill(P, 0.0)
        da = (W * (G @ d @ G)).sum()
        db = al * 2 * T.KP / be ** 3 * (W * (H @ d @ G + G @ d @ H)).sum()
        if up.dpsf is not None:
            g = torch.exp(-T.KP * u * u / be ** 2)
            gg = g.view(-1, 1) * g.view(1, -1)
            gp = up.dpsf[b].double()
            da = da + (gp * gg).sum()
            db = db + al * 2 * T.KP / be ** 3 * (gp * gg * (u.view(-1, 1) ** 2 + u.view(1, -1) ** 2)).sum()
        dab[b, 0], dab[b, 1] = da, db
        dd[b] = al * (G @ W @ G)
    return Grads(dab, dd)


# ------------------------------------------------------------------------------------------------------ depth-gradient impulses
def impulse_depth():
    """One positive depth image for all impulses; its maximum (the plateau: one pixel) lies on none of the impulse positions."""
    g = torch.Generator().manual_seed(7100)
    d = torch.rand(100, 100, generator=g) * 5
    d[20, 20] = 6.0
    return d


def impulse_inputs():
    """(depth (B,100,100), ab (B,3), dHR (B,100,100)): dHR of sample i is IMPULSE_VALUES[i % 3] at IMPULSE_ALL[i], 0 elsewhere."""
    B = len(T.IMPULSE_ALL)
    dHR = torch.zeros(B, 100, 100)
    for i, (y, x) in enumerate(T.IMPULSE_ALL):
        dHR[i, y, x] = T.impulse_value(i)
    ab = torch.tensor([T.impulse_params(i) for i in range(B)])
    return impulse_depth().unsqueeze(0).repeat(B, 1, 1), ab, dHR


def impulse_dd_closed_form(i):
    """alpha v g(y - y0) g(x - x0), exactly 0 beyond +-49; fp64 from the fp32 numbers the kernel receives."""
    y0, x0 = T.IMPULSE_ALL[i]
    a, b, _ = (float(torch.tensor(t, dtype=torch.float32)) for t in T.impulse_params(i))
    v = float(torch.tensor(T.impulse_value(i), dtype=torch.float32))
    k = torch.arange(100, dtype=torch.float64)
    gy = torch.where((k - y0).abs() <= 49, T.gauss_tap(b, k - y0), torch.zeros((), dtype=torch.float64))
    gx = torch.where((k - x0).abs() <= 49, T.gauss_tap(b, k - x0), torch.zeros((), dtype=torch.float64))
    return a * v * gy.view(-1, 1) * gx.view(1, -1)


def transposed_pairs():
    """[(i, j)]: impulse j sits at the transposed position of impulse i, i < j, both under the same (alpha, beta, gamma)."""
    pos = {p: i for i, p in enumerate(T.IMPULSE_ALL)}
    return [(i, pos[(x, y)]) for i, (y, x) in enumerate(T.IMPULSE_ALL)
            if y != x and (x, y) in pos and i < pos[(x, y)] and T.impulse_params(i) == T.impulse_params(pos[(x, y)])]


# ------------------------------------------------------------------------------------------------------------ plateau semantics
PLATEAU_VALUE = 1e30


def plateau_inputs():
    """The degenerate case (all-plateau images, block plateaus on tile 3 and the last wave, three levels) with its own dLR_deg,
    positive dpsf and two dHR: all zero, and 1e30 on the plateau pixels only."""
    case = T.degenerate_case()
    _, dpsf = upstream("degenerate", "positive")
    P = case.depth > case.depth.amax(dim=(1, 2), keepdim=True) - 1e-3
    zero = torch.zeros_like(case.depth)
    return case, dpsf, zero, zero.masked_fill(P, PLATEAU_VALUE), P


# ----------------------------------------------------------------------------------------------------- persistent walks, isolation
def walk_upstream(B, seed):
    """Non-negative dHR (x 1e-4) and dpsf for a large batch."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 100, 100, generator=g) + 0.1) * HR_UP_SCALE, torch.rand(B, 99, 99, generator=g) + 0.1


ISOLATION_SEED, WALK_SEED = 7200, 7300


def walk_rows(depth, margin=2e-7):
    """The samples of a large random batch whose every pixel keeps `margin` from the plateau threshold: on the others (14 of the
    2100 of _persistent_loops.tpsf_inputs have a pixel within 2e-7 of depth.max() - 1e-3) the fp32 kernel and the fp64 yardstick
    may put that pixel on different sides, which is no error of either."""
    m = torch.tensor([T.plateau_margin(depth[i:i + 1]) for i in range(depth.shape[0])])
    return (m > margin).nonzero().flatten()


def isolation_inputs(poisoned):
    """_tpsf_cases.isolation_inputs(False) (B = 600, every grid walks) with dHR and dpsf; poisoned: samples 0..5 carry a NaN or
    +Inf in dHR, 6..10 in dpsf, 11..15 in the depth (on the wave seams and tile 3 as well)."""
    depth, ab, dl = T.isolation_inputs(False)
    dHR, dpsf = walk_upstream(T.ISOLATION_B, ISOLATION_SEED)
    if poisoned:
        spots = [(0, 0), (31, 50), (96, 96), (99, 99), (50, 49), (64, 95)]
        for b in range(6):
            dHR[b][spots[b]] = T.NAN if b % 2 == 0 else float("inf")
        for b in range(6, 11):
            dpsf[b, (b * 17) % 99, (b * 29) % 99] = T.NAN if b % 2 == 0 else float("-inf")
        for b in range(11, 16):
            depth[b][spots[b - 11]] = T.NAN if b % 2 == 0 else float("inf")
    return depth, ab, dl, dHR, dpsf


# ----------------------------------------------------------------------------------------------------------------------- module
MOD_B = 5


def module_inputs():
    g = torch.Generator().manual_seed(7400)
    x = torch.rand(MOD_B, 3, 4, 4, generator=g) * 8
    depth = torch.rand(MOD_B, 100, 100, generator=g) * 3
    depth[1, 40:60, 30:70] = 4.0                                 # a block plateau
    depth[2] = (depth[2] > 2.1).float()                          # a binary contact map, as the datasets hold
    w1 = torch.randn(MOD_B, 1, 100, 100, generator=g) * 1e-4
    z = torch.rand(MOD_B, 1, 4, 4, generator=g)
    w2 = torch.randn(MOD_B, 1, 99, 99, generator=g) * 1e-3
    w3 = torch.randn(MOD_B, 1, 3, generator=g)
    return x, depth, w1, z, w2, w3


# --------------------------------------------------------------------------------------------------------------------- refusals
def refusal_table_ex(p):
    """[(label, ctypes argument list)] of tpsf_backward_ex: every call must return 1 before any HIP call."""
    I, N0 = ctypes.c_int, ctypes.c_void_p(0)
    B = T.REFUSAL_TPSF_B
    names = ["depth", "ab", "HR", "dl", "dHR", "dpsf", "dab", "dd", "work"]
    rows = []
    for k, nm in enumerate(names):
        if nm in ("depth", "ab", "HR", "dab", "work"):
            rows.append((f"NULL {nm}", [N0 if j == k else p(n) for j, n in enumerate(names)] + [I(B), N0]))
    rows.append(("no upstream gradient", [N0 if n in ("dl", "dHR", "dpsf") else p(n) for n in names] + [I(B), N0]))
    rows.append(("no upstream gradient, no d_depth", [N0 if n in ("dl", "dHR", "dpsf", "dd") else p(n) for n in names] + [I(B), N0]))
    for bad in (0, -1):
        rows.append((f"B={bad}", [p(n) for n in names] + [I(bad), N0]))
    return rows
