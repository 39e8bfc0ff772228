"""Kernel-level tests of tpsf_forward / tpsf_backward (csrc/tpsf_mfma.hip) sample by sample and component by component, and of
the refusals and empty splits of the tsr_sgemm family (csrc/sgemm_mfma.hip).

Yardstick, rule, case tables: tests/_tpsf_cases.py (preconditions checked on the CPU by tests/test_tpsf_cases_cpu.py).  Every
comparison against fp64 is   |kernel - fp64| <= max(1e-5 * scale, 4 * |fp32 oracle - fp64|)   element by element, with the scale
named at each check -- the quantity's own, never the batch's.  Exact expectations (== 0, torch.equal) are exact.  Every output
buffer is NaN-prefilled and carries a NaN guard band of one more sample behind element B, which must still be NaN afterwards.

  1. impulses           one bright pixel under a wide PSF (band-edge tap 0.61): closed form, exact zeros beyond +-49, the fill
                        value, exact symmetry; on the wave seams (rows 31|32, 63|64, 95|96), the last wave's rows 96..99 and
                        column tile 3 (x = 96..99)
  2. conditioned        every gradient component against ITSELF, every LR_deg against its sample
  3. signed             the first 12 samples of test_tpsf_kernels_wide_dynamic_range_batch, each against itself
  4. degenerate         all-plateau images, an all-but-one plateau, all-negative depth, a three-level depth, block plateaus on the
                        tile-3 columns and the last wave's rows
  5. corners            alpha, beta, gamma at the ends of what Softplus emits
  6. isolation          B = 600: NaN / Inf in samples 0..15 leave every other sample bit-identical (persistent loops)
  7. refusals           every refused call returns 1 and leaves its outputs untouched
  8. empty splits       nsplit above the number of K steps: trailing partials are written, as exact zeros
"""
import functools
from collections import namedtuple

import pytest
import torch

import _tpsf_cases as T

pytestmark = pytest.mark.gpu
NAN = float("nan")
Out = namedtuple("Out", "HR LR psf dab work")


def launch(depth, ab, dl):
    """tpsf_forward + tpsf_backward on B samples; outputs NaN-prefilled with one sample of guard band each."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    B = depth.shape[0]
    d, a_, dl_ = depth.contiguous().cuda(), ab.contiguous().cuda(), dl.contiguous().cuda()
    HR = torch.full((B + 1, 100, 100), NAN, device="cuda")
    LR = torch.full((B + 1, 16), NAN, device="cuda")
    psf = torch.full((B + 1, 99, 99), NAN, device="cuda")
    dab = torch.full((B + 1, 3), NAN, device="cuda")
    work = torch.full((B + 1, 100, 100), NAN, device="cuda")
    call("tpsf_forward", ptr(d), ptr(a_), ptr(HR), ptr(LR), ptr(psf), I(B), stream())
    call("tpsf_backward", ptr(d), ptr(a_), ptr(HR), ptr(dl_), ptr(dab), ptr(work), I(B), stream())
    torch.cuda.synchronize()
    out = [t.cpu() for t in (HR, LR, psf, dab, work)]
    for t in out:
        assert bool(torch.isnan(t[B:]).all())               # the guard band
    return Out(*(t[:B] for t in out))


@functools.lru_cache(maxsize=None)
def run_case(name):
    """One launch per case, shared by the tests of that case (never modified)."""
    case = T.CASES[name]()
    return case, launch(case.depth, case.ab, case.dl)


def check_forward(name, case, out, rows=None):
    """HR, LR_deg and psf of the fp32_idx samples under the rule, each against its own sample's maximum."""
    rows = case.fp32_idx if rows is None else rows
    ref, r32 = T.reference64(case, rows), T.fp32_reference(name)
    sel = [case.fp32_idx.index(i) for i in rows]
    idx = torch.tensor(rows)
    T.check(f"{name} HR", out.HR[idx], ref.HR, T.sample_scale(ref.HR), r32.HR[sel])
    T.check(f"{name} LR_deg", out.LR[idx], ref.LR, T.sample_scale(ref.LR), r32.LR[sel])
    T.check(f"{name} psf", out.psf[idx], ref.psf, T.sample_scale(ref.psf), r32.psf[sel])
    return ref, r32, idx, sel


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------- 1. impulses
def test_impulse_forward_closed_form_zeros_fill_and_symmetry():
    """Depth = one pixel of value v (1, 3e-3, 2e4), (alpha, beta, gamma) = (0.7, 10, 1.3) and two samples at beta = 0.05.
    HR = alpha v g(y - y0) g(x - x0) against each sample's own maximum (all 23 samples at 1e-5, the 12 with an fp32 reference
    under the rule); EXACTLY 0 beyond +-49 of the impulse (one Toeplitz tap too many or too few, or a table shifted by one,
    shows here at 0.61 of the peak); the impulse pixel -- the plateau -- holds the largest HR of the other pixels bit for bit;
    diagonal impulses give a bit-symmetric HR; psf is bit-symmetric and meets alpha g(u) g(v)."""
    case, out = run_case("impulse")
    B = len(T.IMPULSE_ALL)
    cf = torch.stack([T.impulse_closed_form(i) for i in range(B)])
    r32 = T.fp32_reference("impulse")
    T.check("impulse HR vs closed form", out.HR, cf, T.sample_scale(cf), r32.HR, case.fp32_idx)
    pcf = T.psf_closed_form(case.ab)
    T.check("impulse psf vs closed form", out.psf, pcf, T.sample_scale(pcf), r32.psf, case.fp32_idx)
    ref = T.reference64(case, case.fp32_idx)
    T.check("impulse LR_deg", out.LR[torch.tensor(case.fp32_idx)], ref.LR, T.sample_scale(ref.LR), r32.LR)
    k = torch.arange(100)
    for i, (y0, x0) in enumerate(T.IMPULSE_ALL):
        far = ((k - y0).abs() > 49).view(-1, 1) | ((k - x0).abs() > 49).view(1, -1)
        assert bool(far.any()) and bool((out.HR[i][far] == 0).all()), (i, y0, x0)
        others = out.HR[i].clone()
        others[y0, x0] = -1.0
        assert float(out.HR[i, y0, x0]) > 0 and bits(out.HR[i, y0, x0]) == bits(others.max()), (i, y0, x0)
        nb = [(y0 + dy, x0 + dx) for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)) if 0 <= y0 + dy < 100 and 0 <= x0 + dx < 100]
        assert any(bits(out.HR[i, y, x]) == bits(out.HR[i, y0, x0]) for y, x in nb), (i, y0, x0)
        if y0 == x0:
            assert torch.equal(out.HR[i], out.HR[i].t()), (i, y0, x0)
    assert torch.equal(out.psf, out.psf.transpose(1, 2))
    assert bool(torch.isfinite(out.HR).all()) and bool(torch.isfinite(out.LR).all())


def test_impulse_backward_plateau_weight_and_gradient_components():
    """Three more impulses ((40,60), (97,3), (64,96)) with a dense positive dLR_deg: the plateau pixel's dL/dHR in `work` is
    exactly 0 (for all 23 impulses) and nothing else is; each of d/dalpha, d/dbeta, d/dgamma meets fp64 against ITSELF."""
    case, out = run_case("impulse")
    for i, (y0, x0) in enumerate(T.IMPULSE_ALL):
        assert float(out.work[i, y0, x0]) == 0.0, i
        assert int((out.work[i] == 0).sum()) == 1 and bool(torch.isfinite(out.work[i]).all()), i
    rows = T.IMPULSE_BACKWARD
    ref = T.reference64(case, rows)
    r32 = T.fp32_reference("impulse")
    sel = [case.fp32_idx.index(i) for i in rows]
    T.check("impulse d(alpha, beta, gamma), per component", out.dab[torch.tensor(rows)], ref.dab, ref.dab.abs(), r32.dab[sel])


# ---------------------------------------------------------------------------------------------------------- 2. conditioned
def test_conditioned_inputs_every_gradient_component_against_itself():
    """12 samples, depth in [0, 10) x 10^k for k = -3 .. 2, dLR_deg = |randn| + 0.1: d/dalpha and d/dbeta are sums of
    like-signed terms and no component is below 4 % of its row's largest (CPU test), so every dab[b][j] is held to
    1e-5 |ref[b][j]| (or 4 x the fp32 reference's own error on it), every LR_deg to its sample's maximum."""
    case, out = run_case("conditioned")
    ref, r32, idx, sel = check_forward("conditioned", case, out)
    T.check("conditioned d(alpha, beta, gamma), per component", out.dab[idx], ref.dab, ref.dab.abs(), r32.dab[sel])
    for j, nm in enumerate(("alpha", "beta", "gamma")):
        e = ((out.dab[idx].double() - ref.dab).abs() / ref.dab.abs())[:, j].max()
        e32 = ((r32.dab[sel] - ref.dab).abs() / ref.dab.abs())[:, j].max()
        print(f"[tpsf kernels] conditioned d/d{nm}: kernel {float(e):.1e}, fp32 reference {float(e32):.1e}")


# --------------------------------------------------------------------------------------------------------------- 3. signed
def test_signed_inputs_every_sample_against_itself():
    """The first 12 samples of test_tpsf_kernels_wide_dynamic_range_batch (signed dLR_deg; depth x 1e-3; signed, large depth; a
    block plateau), which that test compares jointly against the batch's largest entry: here HR, LR_deg and psf against the
    sample's own maximum and the gradient against the sample's own largest component."""
    case, out = run_case("signed")
    ref, r32, idx, sel = check_forward("signed", case, out)
    T.check("signed d(alpha, beta, gamma), per sample", out.dab[idx], ref.dab, ref.dab.abs().amax(dim=1, keepdim=True),
            r32.dab[sel])


# ----------------------------------------------------------------------------------------------------------- 4. degenerate
def test_degenerate_plateaus():
    """constant 3.0 and all-zero depth: everything is plateau, the fill is max(nothing, 0) = 0: HR, LR_deg and the three
    gradients are exactly 0, psf is still right.  Zeros with one pixel at -5: all BUT that pixel is plateau, HR is alpha * -5
    there and exactly 0 elsewhere.  All-negative depth: the fill is 0.  Three levels max, max - 5e-4 (inside the plateau),
    max - 2e-3 (outside).  Block plateaus over rows 30..34 x columns 94..99 (column tile 3) and rows 95..99 x columns 0..40 (the
    last wave's rows and the seam before them).  All against fp64 under the rule; all plateau pixels hold one bit pattern."""
    case, out = run_case("degenerate")
    ref, r32, idx, sel = check_forward("degenerate", case, out)
    T.check("degenerate d(alpha, beta, gamma), per sample", out.dab, ref.dab, ref.dab.abs().amax(dim=1, keepdim=True), r32.dab)
    name = {n: i for i, n in enumerate(T.DEGENERATE)}
    for n in ("constant", "zeros"):
        i = name[n]
        assert bool((out.HR[i] == 0).all()) and bool((out.LR[i] == 0).all()) and bool((out.dab[i] == 0).all()), n
        assert bool((out.work[i] == 0).all()), n
        assert bool((ref.HR[i] == 0).all()) and bool((ref.dab[i] == 0).all())
    i = name["spike"]
    y0, x0 = T.SPIKE_AT
    rest = out.HR[i].clone()
    rest[y0, x0] = 0.0
    assert bool((rest == 0).all())
    want = float(case.ab[i, 0].double() * T.SPIKE_VALUE)
    assert abs(float(out.HR[i, y0, x0]) - want) <= 1e-5 * abs(want)
    assert int((out.work[i] != 0).sum()) == 1 and float(out.work[i, y0, x0]) != 0.0
    assert float(out.dab[i, 1]) == 0.0 and float(ref.dab[i, 1]) == 0.0          # g(0) = 1 whatever beta is
    i = name["negative"]
    m = case.depth[i] > case.depth[i].max() - 1e-3
    assert bool((out.HR[i][m] == 0).all()) and bool((out.HR[i][~m] < 0).all())
    for n in T.DEGENERATE:
        i = name[n]
        m = case.depth[i] > case.depth[i].max() - 1e-3
        assert bits(out.HR[i][m]).unique().numel() == 1, n
        assert bool((out.work[i][m] == 0).all()), n
    assert int((case.depth[name["levels"]] > T.LEVEL_MAX - 1e-3).sum()) > 6000
    assert bool(torch.isfinite(out.HR).all()) and bool(torch.isfinite(out.dab).all())


# -------------------------------------------------------------------------------------------------------------- 5. corners
@pytest.mark.parametrize("name", ["corners_positive", "corners_signed"])
def test_parameter_corners(name):
    """alpha in {1e-3, 50} x beta in {0.03, 30} x gamma in {0.05, 50}: beta = 0.03 leaves one tap (g(1) = 1e-10, fp16 planes
    flush it), beta = 30 a nearly flat 99-tap filter whose row sums reach the `gbound` clamp; gamma = 0.05 gives mn = 0 exactly,
    gamma = 50 mn = 0.135.  HR, LR_deg and psf against the sample's maximum, the gradient against the row's largest component
    (at beta = 0.03 d/dbeta is 1e-10 of the others); everything finite."""
    case, out = run_case(name)
    for t in out:
        assert bool(torch.isfinite(t).all())
    ref, r32, idx, sel = check_forward(name, case, out)
    T.check(f"{name} d(alpha, beta, gamma), per sample", out.dab, ref.dab, ref.dab.abs().amax(dim=1, keepdim=True), r32.dab)


# ------------------------------------------------------------------------------------------------------------ 6. isolation
def test_nan_and_inf_samples_leave_the_rest_of_the_batch_bit_identical():
    """B = 600: forward workgroups 0..87 and every tpsf_bwd_dhb workgroup run later iterations.  Second run: samples 0..7 have a
    NaN or +Inf depth pixel, samples 8..15 a NaN alpha, beta or gamma -- samples 512..527 then follow a poisoned sample in their
    forward workgroup, 256..271 and 512..527 in their tpsf_bwd_dhb workgroup.  HR, LR_deg, psf and the gradients of samples
    16..599 are bit-identical between the two runs (LDS tables, masks, reduction slots and prefetched rows carry nothing
    over)."""
    n = T.ISOLATION_POISONED
    clean = launch(*T.isolation_inputs(False))
    for t in clean:
        assert bool(torch.isfinite(t).all())
    dirty = launch(*T.isolation_inputs(True))
    for q in ("HR", "LR", "psf", "dab"):
        assert torch.equal(getattr(clean, q)[n:], getattr(dirty, q)[n:]), q
    assert not bool(torch.isfinite(dirty.LR[:n]).all(dim=1).any())                # the poison did reach its own samples


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refused_calls_return_1_and_leave_the_outputs_untouched():
    """NULL pointers, B <= 0, M / N / K <= 0, unknown activations, nsplit outside 1..65535 and a split stride below the partial's
    size: status 1, nothing launched, every buffer still NaN."""
    from tactilesr_amd._lib import load, ptr
    lib = load()
    M, N, K = T.REFUSAL_MNK
    B = T.REFUSAL_TPSF_B
    shapes = {"depth": (B, 100, 100), "ab": (B, 3), "HR": (B, 100, 100), "LRd": (B, 16), "psf": (B, 99, 99), "dl": (B, 16),
              "dab": (B, 3), "work": (B, 100, 100), "A": (M, K), "Bm": (K, N), "C": (M, N), "bias": (N,), "slab": (4, M, N)}
    buf = {k: torch.full(s, NAN, device="cuda") for k, s in shapes.items()}
    for label, fn, args in T.refusal_table(lambda name: ptr(buf[name])):
        assert getattr(lib, fn)(*args) == 1, label
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool(torch.isnan(t).all()), k


# --------------------------------------------------------------------------------------------------------- 8. empty splits
def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("M,N,K,ns", T.EMPTY_SPLIT_SHAPES)
def test_splitk_with_more_splits_than_k_steps_writes_zero_partials(M, N, K, ns):
    """A split's K range is ceil(K / nsplit) rounded up to whole 32-deep K steps, so with nsplit above the number of K steps the
    trailing splits are empty: they still write their partial, as exact zeros, into a NaN-prefilled slab, and tsr_reduce_splits
    over ALL nsplit partials meets fp64 at 2e-6.  Contiguous and strided slabs; the gap of the strided slab stays NaN."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_longlong as L, c_float as Fl
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    A, Bm = torch.randn(M, K, generator=g).cuda(), torch.randn(K, N, generator=g).cuda()
    ref = A.double().cpu() @ Bm.double().cpu()
    live = T.nonempty_splits(K, ns)
    assert live < ns
    slab = torch.full((ns + 1, M, N), NAN, device="cuda")
    call("tsr_sgemm_splitk", ptr(A), L(K), L(1), ptr(Bm), L(N), L(1), ptr(slab), I(M), I(N), I(K), I(ns), stream())
    out = torch.full((M * N + 8,), NAN, device="cuda")
    call("tsr_reduce_splits", ptr(slab), ptr(out), L(M * N), I(ns), Fl(1.0), stream())
    assert not bool(torch.isnan(slab[:ns]).any()) and bool(torch.isnan(slab[ns]).all())
    assert bool((slab[live:ns] == 0).all()) and bool((slab[:live] != 0).flatten(1).any(dim=1).all())
    assert _relerr(out[:M * N].view(M, N), ref) < 2e-6 and bool(torch.isnan(out[M * N:]).all())
    gap, tot = 24, M * N + 24
    slab = torch.full(((ns + 1) * tot,), NAN, device="cuda")
    call("tsr_sgemm_splitk_strided", ptr(A), L(K), L(1), ptr(Bm), L(N), L(1), ptr(slab), L(tot), I(M), I(N), I(K), I(ns),
         stream())
    sl = slab.view(ns + 1, tot)
    assert not bool(torch.isnan(sl[:ns, :M * N]).any()) and bool((sl[live:ns, :M * N] == 0).all())
    assert bool(torch.isnan(sl[:ns, M * N:]).all()) and bool(torch.isnan(sl[ns]).all()) and gap == tot - M * N
    out = torch.full((tot,), NAN, device="cuda")
    call("tsr_reduce_splits", ptr(slab), ptr(out), L(tot), I(ns), Fl(1.0), stream())
    assert _relerr(out[:M * N].view(M, N), ref) < 2e-6


def test_colsum_splitk_with_more_splits_than_rows_writes_zero_partials():
    from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_longlong as L, c_float as Fl
    M, N, ns = T.EMPTY_COLSUM
    g = torch.Generator().manual_seed(77)
    Y = torch.randn(M, N, generator=g).cuda()
    live = T.nonempty_splits(M, ns)
    tot = N + 10
    slab = torch.full(((ns + 1) * tot,), NAN, device="cuda")
    call("tsr_colsum_splitk", ptr(Y), ptr(slab), L(tot), I(M), I(N), I(ns), stream())
    sl = slab.view(ns + 1, tot)
    assert not bool(torch.isnan(sl[:ns, :N]).any()) and bool((sl[live:ns, :N] == 0).all())
    assert bool(torch.isnan(sl[:ns, N:]).all()) and bool(torch.isnan(sl[ns]).all())
    out = torch.full((tot,), NAN, device="cuda")                  # partials lie `tot` apart: the gap is reduced along (NaN)
    call("tsr_reduce_splits", ptr(slab), ptr(out), L(tot), I(ns), Fl(1.0), stream())
    assert _relerr(out[:N], Y.double().cpu().sum(0)) < 2e-6 and bool(torch.isnan(out[N:]).all())
