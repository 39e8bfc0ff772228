"""Preconditions of tests/test_gpu_tpsf_kernels.py, checked without a device: the fp64 matrix-form yardstick of
tests/_tpsf_cases.py agrees with the oracle's direct convolution; every case table keeps its pixels away from the plateau
threshold, stays within the sizes the GPU tests promise, and keeps the fp32-reference term of the comparison rule below its cap;
the conditioned case's gradient components are all far from zero; the refused calls are refused before any HIP call."""
import ctypes

import pytest
import torch

import _tpsf_cases as T


def _rel(a, b):
    """max |a - b| per sample over that sample's max |b|, worst sample."""
    return float(((a - b).abs().flatten(1).amax(dim=1) / b.abs().flatten(1).amax(dim=1).clamp_min(1e-300)).max())


def test_matrix_form_agrees_with_the_oracle_in_fp64():
    """A random sample, the signed one and the block plateau of the signed case, and one impulse: HR, LR_deg, psf and the
    gradients within 1e-6 of the oracle's direct 99x99 convolution in fp64 (measured: below 1e-7, what the oracle's fp32
    geometry tables leave), each normalised by the sample's own maximum."""
    for name, idx in (("signed", [0, 2, 3]), ("impulse", [4])):
        case = T.CASES[name]()
        mine = T.reference64(case, idx)
        ora = T.oracle_reference(case, idx, torch.float64)
        for q in T.Ref._fields:
            e = _rel(getattr(mine, q), getattr(ora, q))
            print(f"[tpsf cases] {name} {q}: matrix form vs oracle fp64 {e:.1e}")
            assert e < 1e-6, (name, q, e)


def test_impulse_closed_form_is_the_yardstick_on_impulses():
    """The closed form the GPU test compares HR with is what forward64 gives for the same input, to fp64 rounding; it is exactly
    0 beyond +-49 of the impulse and its plateau pixel holds the largest other value."""
    case = T.impulse_case()
    ref = T.reference64(case)
    for i, (y0, x0) in enumerate(T.IMPULSE_ALL):
        cf = T.impulse_closed_form(i)
        assert float((cf - ref.HR[i]).abs().max()) <= 1e-12 * float(cf.max()), i
        k = torch.arange(100)
        far = ((k - y0).abs() > 49).view(-1, 1) | ((k - x0).abs() > 49).view(1, -1)
        assert bool((cf[far] == 0).all()) and bool((ref.HR[i][far] == 0).all())
        assert int((case.depth[i] != 0).sum()) == 1 and float(case.depth[i, y0, x0]) > 1e-3
    assert float((T.psf_closed_form(case.ab) - ref.psf).abs().max()) < 1e-15
    assert [T.impulse_value(i) for i, (y, x) in enumerate(T.IMPULSE_ALL) if y == x] == [1.0, 1.0, 1.0]
    assert T.gauss_tap(10.0, 49) > 0.6                      # the band-edge tap is 61 % of the centre
    assert [T.impulse_params(i) for i in (17, 18, 19, 20)] == [T.IMPULSE_WIDE, T.IMPULSE_NARROW, T.IMPULSE_NARROW, T.IMPULSE_WIDE]


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_tables_sizes_and_plateau_margins(name):
    case = T.CASES[name]()
    B = case.depth.shape[0]
    assert B <= 64 and case.depth.shape == (B, 100, 100) and case.ab.shape == (B, 3) and case.dl.shape == (B, 16)
    assert case.depth.dtype == case.ab.dtype == case.dl.dtype == torch.float32
    assert len(case.fp32_idx) <= T.MAX_FP32_SAMPLES and max(case.fp32_idx) < B
    # every pixel keeps its distance from the threshold; the one exception is the maximum pixel of the 2e4 impulses, whose 1e-3
    # is 5e-8 of 2e4: there the fp32 comparison is evaluated exactly instead
    big = case.depth.amax(dim=(1, 2)) > 5000
    assert name == "impulse" or not bool(big.any())
    assert T.plateau_margin(case.depth[~big]) > 2e-7
    if bool(big.any()):
        assert T.plateau_margin(case.depth[big], skip_max=True) > 2e-7
    assert T.max_pixel_is_on_the_fp32_plateau(case.depth)
    assert bool(torch.isfinite(case.depth).all()) and bool((case.ab > 0).all())


def test_isolation_inputs():
    depth, ab, dl = T.isolation_inputs(False)
    pd, pab, pdl = T.isolation_inputs(True)
    B, n = T.ISOLATION_B, T.ISOLATION_POISONED
    assert depth.shape[0] == B and T.FWD_GRID < B < 2 * T.FWD_GRID and B > 2 * T.DHB_GRID and n <= B - T.FWD_GRID
    assert torch.equal(depth[n:], pd[n:]) and torch.equal(ab[n:], pab[n:]) and torch.equal(dl, pdl)
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(ab).all())
    for b in range(8):
        assert int((~torch.isfinite(pd[b])).sum()) == 1 and bool(torch.isfinite(pab[b]).all())
    for b in range(8, 16):
        assert int(torch.isnan(pab[b]).sum()) == 1 and bool(torch.isfinite(pd[b]).all())
    assert {int(torch.isnan(pab[b]).nonzero()) for b in range(8, 16)} == {0, 1, 2}
    assert T.plateau_margin(depth) > 2e-7


def test_conditioned_gradient_components_are_far_from_zero():
    """Every d/d(alpha, beta, gamma) of the conditioned case is at least 1e-2 of its row's largest: a bar relative to the
    component itself says something about each of them."""
    ref = T.reference64(T.conditioned_case())
    ratio = ref.dab.abs() / ref.dab.abs().amax(dim=1, keepdim=True)
    print(f"[tpsf cases] conditioned: smallest gradient component {float(ratio.min()):.3f} of its row's largest")
    assert float(ratio.min()) >= 1e-2
    assert bool((ref.dab[:, :2] > 0).all())                 # like-signed sums


def _scales(name, ref):
    """The scale of every check the GPU tests make on the case `name`, for the rows `ref` holds: [(label, ref tensor, scale)]."""
    rowmax = ref.dab.abs().amax(dim=1, keepdim=True)
    out = [("HR", ref.HR, T.sample_scale(ref.HR)), ("LR_deg", ref.LR, T.sample_scale(ref.LR)),
           ("psf", ref.psf, T.sample_scale(ref.psf))]
    if name in ("conditioned", "impulse"):
        out.append(("dab", ref.dab, ref.dab.abs()))
    else:
        out.append(("dab", ref.dab, rowmax))
    return out


@pytest.mark.parametrize("name", list(T.CASES))
def test_fp32_reference_term_stays_below_its_cap(name):
    """4 x |fp32 oracle - fp64| is below 1e-3 of the scale for every element the GPU tests compare under the rule: the second
    term widens a bar to at most a thousandth of the quantity, so no element is effectively unchecked."""
    case = T.CASES[name]()
    idx = case.fp32_idx
    if name == "impulse":
        idx = T.IMPULSE_BACKWARD                             # gradients are compared on these only
    ref = T.reference64(case, case.fp32_idx)
    r32 = T.fp32_reference(name)
    for (label, r64, scale), q in zip(_scales(name, ref), T.Ref._fields):
        term = T.FP32_FACTOR * (getattr(r32, q) - r64).abs()
        den = scale.expand_as(r64)
        if label == "dab" and name == "impulse":
            rows = [case.fp32_idx.index(i) for i in idx]
            term, den = term[rows], den[rows]
        ok = term <= T.FP32_CAP * den
        worst = float((term / den.clamp_min(1e-300)).max())
        print(f"[tpsf cases] {name} {label}: fp32-reference term at most {worst:.1e} of the scale")
        assert bool(ok.all()), (name, label, worst)


def test_split_arithmetic_of_the_empty_split_cases():
    for M, N, K, ns in T.EMPTY_SPLIT_SHAPES:
        assert T.splitk_chunk(K, ns) % T.SG_KT == 0 and 1 <= T.nonempty_splits(K, ns) < ns
    assert [T.nonempty_splits(K, ns) for _, _, K, ns in T.EMPTY_SPLIT_SHAPES] == [1, 1, 2]
    M, N, ns = T.EMPTY_COLSUM
    assert T.nonempty_splits(M, ns) == 1


def test_refused_calls_return_1_before_any_hip_call():
    """The argument table of the GPU refusal test with fake non-NULL pointers and no device: every call fails its argument
    check on the host and returns TSR_ERR_ARG = 1."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    rows = T.refusal_table(lambda name: ctypes.c_void_p(16))
    assert len(rows) == 7 + 8 + 11 + 1 + 2 + 3 + 1
    assert len({r[0] for r in rows}) == len(rows)
    for label, fn, args in rows:
        assert len(args) == len(_lib.SIGNATURES[fn]), label
        assert getattr(lib, fn)(*args) == 1, label
