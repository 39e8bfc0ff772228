"""Preconditions of tests/test_gpu_tpsf_autograd.py, checked without a device: the closed forms that tpsf_backward_ex implements
(include/tactilesr_hip.h) are the fp64 autograd of the yardstick; every new input table keeps its pixels away from the plateau
threshold; the fp32-oracle term of the comparison rule stays below its cap for every scenario; tpsf_backward_ex refuses what it
must before any HIP call; the symbol is declared, bound and exported under ABI 24."""
import ctypes
import os
import re

import pytest
import torch

import _tpsf_cases as T
import _tpsf_autograd as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 2e-7                       # the threshold tests/test_tpsf_cases_cpu.py holds the case tables to


@pytest.mark.parametrize("name", A.AG_CASES)
def test_closed_forms_are_the_fp64_autograd_of_the_yardstick(name):
    """d/dalpha, d/dbeta (d/dgamma too where it is an exact 0) and d_depth of the header's formulas against torch.autograd.grad
    through forward64, for every (kind, mode), to 1e-9 of the scale: the sample's largest |d_depth|, the row's largest gradient
    component."""
    case = T.CASES[name]()
    worst = 0.0
    for kind in A.KINDS:
        for mode in A.MODES:
            up = A.scenario_up(name, kind, mode)
            ref = A.grads64(case.depth, case.ab, up)
            cf = A.closed_form(case.depth, case.ab, up)
            cols = [0, 1] if up.dl is not None else [0, 1, 2]
            rowmax = ref.dab.abs().amax(dim=1, keepdim=True)
            e_ab = ((cf.dab - ref.dab).abs() / rowmax.clamp_min(1e-300))[:, cols].max()
            e_dd = ((cf.dd - ref.dd).abs() / T.sample_scale(ref.dd).clamp_min(1e-300)).max()
            worst = max(worst, float(e_ab), float(e_dd))
            assert float(e_ab) <= 1e-9 and float(e_dd) <= 1e-9, (name, kind, mode, float(e_ab), float(e_dd))
            if up.dl is None:
                assert bool((ref.dab[:, 2] == 0).all())
            if mode == "psf":
                assert bool((ref.dd == 0).all())
    print(f"[tpsf autograd cpu] {name}: closed forms vs fp64 autograd {worst:.1e}")


def test_plateau_pixels_of_the_input_receive_a_gradient_and_the_output_plateau_carries_none():
    """On the block plateaus of the degenerate case d_depth under the plateau is non-zero, and a 1e30 in dHR on the plateau
    changes nothing in the fp64 autograd either."""
    case, dpsf, zero, big, P = A.plateau_inputs()
    ref0 = A.grads64(case.depth, case.ab, A.Up(case.dl, zero, dpsf))
    ref1 = A.grads64(case.depth, case.ab, A.Up(case.dl, big, dpsf))
    assert torch.equal(ref0.dab, ref1.dab) and torch.equal(ref0.dd, ref1.dd)
    name = {n: i for i, n in enumerate(T.DEGENERATE)}
    for n in ("block_tile3", "block_lastwave", "levels"):
        i = name[n]
        assert bool(P[i].any()) and bool((ref0.dd[i][P[i]] != 0).all()), n
    for n in ("constant", "zeros"):
        i = name[n]
        assert bool(P[i].all()) and bool((ref0.dd[i] == 0).all()) and bool((ref0.dab[i, :2] != 0).all()), n


def test_new_input_tables_keep_their_plateau_margin():
    from _persistent_loops import tpsf_inputs, TPSF_B
    d, ab, dHR = A.impulse_inputs()
    assert T.plateau_margin(d) > MARGIN
    P = d[0] > d[0].max() - 1e-3
    assert int(P.sum()) == 1 and not any(bool(P[y, x]) for y, x in T.IMPULSE_ALL)
    for i, (y, x) in enumerate(T.IMPULSE_ALL):
        assert int((dHR[i] != 0).sum()) == 1 and float(dHR[i, y, x]) == float(torch.tensor(T.impulse_value(i)))
    assert len(A.transposed_pairs()) >= 3
    for clean in (False, True):
        depth, ab, dl, gHR, gpsf = A.isolation_inputs(not clean)
        assert depth.shape[0] == T.ISOLATION_B
        assert T.plateau_margin(depth[T.ISOLATION_POISONED:]) > MARGIN
    depth, ab, dl, gHR, gpsf = A.isolation_inputs(True)
    c = A.isolation_inputs(False)
    n = T.ISOLATION_POISONED
    for dirty, ok in zip((depth, ab, dl, gHR, gpsf), c):
        assert torch.equal(dirty[n:], ok[n:])
    bad = lambda t: (~torch.isfinite(t)).flatten(1).sum(1)
    assert bad(gHR)[:6].tolist() == [1] * 6 and bad(gpsf)[6:11].tolist() == [1] * 5 and bad(depth)[11:16].tolist() == [1] * 5
    assert int(bad(gHR).sum() + bad(gpsf).sum() + bad(depth).sum()) == 16 and all(bool(torch.isfinite(t).all()) for t in c)
    assert T.plateau_margin(A.module_inputs()[1]) > MARGIN
    wd, wab, wdl = tpsf_inputs()
    from _persistent_loops import TPSF_INDICES, TPSF_POOL_GRID, TPSF_FWD_GRID, TPSF_DHB_GRID
    rows = A.walk_rows(wd, MARGIN)
    assert wd.shape[0] == TPSF_B == 2100 and len(rows) >= 2080 and T.plateau_margin(wd[rows]) > MARGIN
    assert set(TPSF_INDICES) <= set(rows.tolist())
    assert TPSF_B > TPSF_POOL_GRID and TPSF_B > 4 * TPSF_FWD_GRID and TPSF_B > 8 * TPSF_DHB_GRID      # every grid walks
    assert int((rows >= TPSF_POOL_GRID).sum()) > 40 and int((rows >= 4 * TPSF_FWD_GRID).sum()) > 40
    for name in A.AG_CASES:
        assert T.plateau_margin(T.CASES[name]().depth) > MARGIN and max(A.FP32_ROWS[name]) < T.CASES[name]().depth.shape[0]


@pytest.mark.parametrize("name", A.AG_CASES)
def test_fp32_reference_term_stays_below_its_cap(name):
    """4 x |fp32 oracle - fp64| <= 1e-3 of the scale for every scenario of the case, on d(alpha, beta, gamma) and on d_depth."""
    case = T.CASES[name]()
    rows = A.FP32_ROWS[name]
    r32 = A.fp32_grads(name)
    for kind in A.KINDS:
        for mode in A.MODES:
            ref = A.grads64(case.depth, case.ab, A.scenario_up(name, kind, mode), rows)
            g32 = r32[(kind, mode)]
            for label, r64, q32, scale in (("dab", ref.dab, g32.dab, A.dab_scale(name, kind, ref.dab)),
                                           ("d_depth", ref.dd, g32.dd, T.sample_scale(ref.dd))):
                term = T.FP32_FACTOR * (q32 - r64).abs()
                den = scale.expand_as(r64)
                worst = float((term / den.clamp_min(1e-300)).max())
                print(f"[tpsf autograd cpu] {name} {kind} {mode} {label}: fp32-reference term at most {worst:.1e} of the scale")
                assert bool((term <= T.FP32_CAP * den).all()), (name, kind, mode, label, worst)


def test_impulse_closed_form_is_the_yardstick():
    d, ab, dHR = A.impulse_inputs()
    ref = A.grads64(d, ab, A.Up(None, dHR, None))
    k = torch.arange(100)
    for i, (y0, x0) in enumerate(T.IMPULSE_ALL):
        cf = A.impulse_dd_closed_form(i)
        assert float((cf - ref.dd[i]).abs().max()) <= 1e-12 * float(cf.abs().max()), i
        far = ((k - y0).abs() > 49).view(-1, 1) | ((k - x0).abs() > 49).view(1, -1)
        assert bool(far.any()) and bool((cf[far] == 0).all())


def test_tpsf_backward_ex_refuses_before_any_hip_call():
    """Fake non-NULL pointers, no device: every row returns TSR_ERR_ARG = 1 on the host; the all-NULL-upstream rows included."""
    from tactilesr_amd import _lib
    lib = _lib.load()
    rows = A.refusal_table_ex(lambda name: ctypes.c_void_p(16))
    assert len(rows) == 5 + 2 + 2 and len({r[0] for r in rows}) == len(rows)
    for label, args in rows:
        assert len(args) == len(_lib.SIGNATURES["tpsf_backward_ex"]), label
        assert lib.tpsf_backward_ex(*args) == 1, label
    # tpsf_backward keeps its own refusals
    for label, fn, args in T.refusal_table(lambda name: ctypes.c_void_p(16)):
        if fn == "tpsf_backward":
            assert getattr(lib, fn)(*args) == 1, label


def test_tpsf_backward_ex_is_declared_bound_and_exported_under_abi_24():
    from tactilesr_amd import _lib
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    m = re.search(r"int tpsf_backward_ex\(([^;]*)\);", header)
    assert m, "tpsf_backward_ex is not declared in include/tactilesr_hip.h"
    params = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    sig = _lib.SIGNATURES["tpsf_backward_ex"]
    assert len(params) == len(sig) == 11
    assert [("*" in a) for a in params] == [t is ctypes.c_void_p for t in sig]
    assert _lib.ABI_VERSION == 24 and _lib.load().tsr_abi_version() == 24
    assert hasattr(_lib.load(), "tpsf_backward_ex")
    assert len(_lib.SIGNATURES["tpsf_backward"]) == 8                   # tpsf_backward keeps its signature
