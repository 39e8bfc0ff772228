"""No GPU: the preconditions of tests/test_gpu_sgemm.py.  Which kernel form a launch takes is asked of the library itself
(tsr_sgemm_form, the function the launch path calls): the table reaches all 18 instantiations of sgemm_tile_kernel through
tsr_sgemm and every production form through the other entry points; the integer data is exact in fp32; an fp32 emulation of
the reference passes the bars the kernel is held to."""
import os
import re

import pytest
import torch

import _sgemm_cases as S
from tactilesr_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in S.TABLE if c.M * c.N <= 1 << 18]          # the emulation loops over k on the host


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def production_forms(lib, batches):
    forms = {e: set() for e in S.ENTRIES}
    for B in batches:
        for _, _, c in S.production_cases(B):
            forms[c.entry].add(S.query_form(lib, c))
    return forms


def test_form_query_is_declared_bound_exported_and_host_only(lib):
    hdr = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    assert re.search(r"^int tsr_sgemm_form\(long long sa0, long long sa1, long long sb0, long long sb1, int a_align16, "
                     r"int b_align16,\s+int M, int N, int K, int nsplit\);", hdr, re.M)
    assert len(_lib.SIGNATURES["tsr_sgemm_form"]) == 10 and hasattr(lib, "tsr_sgemm_form")
    # the launch path makes its choice through the same function and holds no stride or extent test of its own
    src = open(os.path.join(REPO, "tactilesr_amd", "csrc", "sgemm_mfma.hip")).read()
    body = src[src.index("static int sgemm_dispatch("):src.index('extern "C" int tsr_sgemm(')]
    assert "sgemm_form(" in body and "al16(g.A)" in body and "& 3" not in body and "384" not in body
    assert lib.tsr_sgemm_form(32, 1, 1, 32, 1, 1, 64, 64, 32, 1) == 12811          # answered without a device


def test_form_query_refuses_what_the_launches_refuse(lib):
    q = lambda M, N, K, ns: lib.tsr_sgemm_form(K, 1, N, 1, 1, 1, M, N, K, ns)
    assert q(8, 8, 8, 1) == 12812
    for bad in (0, -1):
        assert q(bad, 8, 8, 1) == 0 and q(8, bad, 8, 1) == 0 and q(8, 8, bad, 1) == 0
    assert q(8, 8, 8, 0) == 0 and q(8, 8, 8, -3) == 0 and q(8, 8, 8, 65536) == 0 and q(8, 8, 8, 65535) == 12812


def test_form_query_tile_height_thresholds(lib):
    """64-row tiles exactly when M > 64 and ceil(N/128) * ceil(M/128) * nsplit < 384 (include/tactilesr_hip.h)."""
    q = lambda M, N, ns: lib.tsr_sgemm_form(4, 1, N, 1, 1, 1, M, N, 4, ns) // 100
    assert (q(64, 128, 1), q(65, 128, 1)) == (128, 64)
    assert (q(128, 128, 383), q(128, 128, 384)) == (64, 128)
    assert (q(129, 129, 95), q(129, 129, 96)) == (64, 128)          # 2 x 2 x 96 = 384
    assert (q(49024, 4, 1), q(49025, 4, 1)) == (64, 128)


def test_form_query_load_paths(lib):
    """Every condition of a 16-B path, one at a time: unit stride, the other stride, the extent, the alignment."""
    f = lambda sa0, sa1, al, M, K: lib.tsr_sgemm_form(sa0, sa1, 2, 2, al, 1, M, 8, K, 1) // 10 % 10
    assert f(8, 1, 1, 8, 8) == 1 and f(12, 1, 1, 8, 8) == 1
    assert f(8, 1, 0, 8, 8) == 0 and f(9, 1, 1, 8, 8) == 0 and f(8, 2, 1, 8, 8) == 0 and f(7, 1, 1, 8, 7) == 0
    assert f(1, 8, 1, 8, 8) == 2 and f(1, 8, 1, 8, 7) == 2 and f(1, 12, 1, 8, 8) == 2
    assert f(1, 8, 0, 8, 8) == 0 and f(1, 10, 1, 8, 8) == 0 and f(1, 7, 1, 7, 8) == 0
    g = lambda sb0, sb1, al, N, K: lib.tsr_sgemm_form(2, 2, sb0, sb1, 1, al, 8, N, K, 1) % 10
    assert g(1, 8, 1, 8, 8) == 1 and g(1, 8, 0, 8, 8) == 0 and g(1, 9, 1, 8, 8) == 0 and g(1, 6, 1, 8, 6) == 0
    assert g(8, 1, 1, 8, 8) == 2 and g(8, 1, 1, 8, 5) == 2 and g(8, 1, 0, 8, 8) == 0 and g(6, 1, 1, 6, 8) == 0


@pytest.mark.parametrize("c", S.TABLE, ids=S.case_id)
def test_every_row_reaches_the_form_it_names(lib, c):
    assert S.query_form(lib, c) == c.form
    assert 0 <= c.a_off <= 3 and 0 <= c.b_off <= 3 and c.entry in S.ENTRIES
    assert c.nsplit == 1 or c.entry.startswith("splitk")


def test_the_table_reaches_all_18_forms_through_tsr_sgemm(lib):
    reached = {S.query_form(lib, c) for c in S.rows("sgemm")}
    print(f"[sgemm cases] tsr_sgemm rows reach {len(reached)}/18 forms: {sorted(reached)}")
    assert reached == set(S.ALL_FORMS) and len(S.ALL_FORMS) == 18
    # both ways into each path: every form has a row whose tile overhangs A's and B's extent or K range (masked-out loads)
    for form in S.ALL_FORMS:
        assert any(all(S.masked_loads(c)) for c in S.rows("sgemm") if c.form == form), form
    # and the generic path is entered in all three ways
    gen = [c for c in S.rows("sgemm") if c.form // 10 % 10 == 0 or c.form % 10 == 0]
    assert any(c.a_off or c.b_off for c in gen) and any(c.a_pad % 4 or c.b_pad % 4 for c in gen)
    assert any(not (c.a_off or c.b_off or c.a_pad or c.b_pad) and "g" not in (c.af, c.bf) for c in gen)      # ragged extent
    assert any("g" in (c.af, c.bf) for c in gen)
    assert any(c.a_pad == 4 and c.form // 10 % 10 and c.b_pad == 4 and c.form % 10 for c in S.rows("sgemm"))


def test_extents_straddle_the_tile_edges():
    t = S.rows("sgemm")
    for v in (1, 63, 64, 65, 127, 128, 129, 130):
        assert any(c.M == v for c in t) and any(c.N == v for c in t), v
    for k in (1, 2, 3, 4, 31, 32, 33, 36, 64, 65, 132):
        assert any(c.K == k for c in S.TABLE), k
    assert all(c.M * c.N <= 6_000_000 for c in S.TABLE)


def test_production_batches_and_forms_are_in_the_table(lib):
    b_dw, b_fwd = S.batch_dw_128(lib), S.batch_fwd_128(lib)
    print(f"[sgemm cases] smallest B with a 128-row dW (M > 64): {b_dw}; with layer 2's forward on 128-row tiles too: {b_fwd}")
    assert 64 < b_dw <= b_fwd
    for B, nm in ((b_dw, "dW1"), (b_fwd, "fwd1")):
        f = {n: S.query_form(lib, c) for n, _, c in S.production_cases(B)}
        g = {n: S.query_form(lib, c) for n, _, c in S.production_cases(B - 1)}
        assert f[nm] // 100 == 128 and g[nm] // 100 == 64
    prod = production_forms(lib, S.PRODUCTION_B + (b_dw, b_fwd))
    for e in S.ENTRIES:
        have = {S.query_form(lib, c) for c in S.rows(e)}
        want = prod[e] | prod["splitk_strided"] if e == "splitk" else prod[e]       # tsr_sgemm_splitk: the same dW forms
        assert want and want <= have, (e, sorted(want - have))
    assert len(S.production_cases(1)) == 12
    # the two production forms the older kernel tests never launched
    assert 12822 in prod["splitk_strided"] and 6402 in prod["masked"]


@pytest.mark.parametrize("entry", ["masked", "splitk", "splitk_strided"])
def test_other_entry_points_cover_the_tile_height_boundaries(lib, entry):
    t = S.rows(entry)
    assert any(c.form // 100 == 128 and c.M > 128 for c in t)
    assert any(c.M == 64 and c.form // 100 == 128 for c in t) and any(c.M == 65 and c.form // 100 == 64 for c in t)
    wg = lambda c: -(-c.N // 128) * -(-c.M // 128) * c.nsplit
    assert any(wg(c) == 383 and c.form // 100 == 64 for c in t) and any(wg(c) == 384 and c.form // 100 == 128 for c in t)
    if entry != "masked":
        assert any(S.nonempty_splits(c.K, c.nsplit) < c.nsplit for c in t)             # empty trailing splits
        assert any((c.K - 1) % S.splitk_chunk(c.K, c.nsplit) == 0 and c.nsplit > 1 for c in t)      # a split holding one k


def test_layouts_place_every_element_and_fill_the_rest_with_nan():
    g = torch.Generator().manual_seed(3)
    for form, ext, K, off, pad in (("k", 5, 7, 2, 3), ("m", 5, 7, 1, 4), ("g", 4, 3, 3, 1), ("k", 3, 1, 0, 0)):
        mat = torch.randn(ext, K, generator=g)
        buf = S.place(mat, form, off, pad)
        size, se, sk = S.layout(form, ext, K, pad)
        assert buf.numel() == off + size
        for e in range(ext):
            for k in range(K):
                assert buf[S.element_index(form, ext, K, pad, off, e, k)] == mat[e, k]
        assert int(torch.isnan(buf).sum()) == buf.numel() - ext * K


@pytest.mark.parametrize("c", S.TABLE, ids=S.case_id)
def test_integer_data_is_exact_in_fp32(c):
    A, B, bias = S.int_data(c)
    assert float(A.abs().max()) <= S.INT_LIMIT and float(B.abs().max()) <= S.INT_LIMIT and c.K <= 4096
    assert all(bool((t == t.round()).all()) for t in (A, B, bias))
    assert S.exactness_margin(A, B, bias) < S.EXACT_LIMIT
    if c.M * c.N <= 1 << 14:
        assert torch.equal(S.emulate32(A, B, bias).double(), S.product64(A, B) + bias.double())


def test_production_integer_data_is_exact_at_the_largest_batch(lib):
    B = S.batch_fwd_128(lib)
    assert max(B, 1024) * S.INT_LIMIT ** 2 + S.INT_LIMIT < S.EXACT_LIMIT


@pytest.mark.parametrize("c", SMALL, ids=S.case_id)
def test_fp32_emulation_of_the_reference_stays_inside_the_bars(c):
    """The bars do not fail the reference alone: sequential fp32 accumulation, every epilogue, every split."""
    A, B, bias = S.normal_data(c)
    worst = 0.0
    if c.entry in ("sgemm", "masked"):
        ab = S.absproduct64(A, B)
        for act, bs in ((0, None), (0, bias), (1, bias), (2, bias), (2, None)):
            pre = S.product64(A, B) + (0 if bs is None else bs.double())
            bar = S.rounded_bar(c.K, ab, None if bs is None else bs.abs(), pre, act)
            el, gl = S.ratios(S.emulate32(A, B, bs, act), S.epilogue64(pre, act), bar)
            assert el <= 1.0 and gl < S.GLOBAL_BAR, (act, el, gl)
            worst = max(worst, el)
    else:
        for k0, k1 in S.split_ranges(c.K, c.nsplit):
            if k0 >= k1:
                continue
            el, gl = S.ratios(S.emulate32(A, B, k0=k0, k1=k1), S.product64(A, B, k0, k1),
                              S.dot_bound(k1 - k0, S.absproduct64(A, B, k0, k1)))
            assert el <= 1.0 and gl < S.GLOBAL_BAR, (k0, el, gl)
            worst = max(worst, el)
    print(f"[sgemm cases] {S.case_id(c)}: fp32 emulation at {worst:.3f} of the elementwise bar")


def test_softplus_probe_grid_and_yardstick():
    A, Bv, bias = S.probe_inputs()
    pre = (Bv + bias).double().view(-1)                      # one fp32 add of exactly representable values
    assert float(pre.min()) <= -109 and float(pre.max()) >= 89
    assert bool(((pre > 19.9) & (pre < 20)).any()) and bool(((pre > 20) & (pre < 20.1)).any()) and bool((pre == 20).any())
    assert bool(((Bv.double() + bias.double()).view(-1) == pre).all()) and torch.equal(pre.float(), S.probe_grid())
    got = S.emulate32(A, Bv, bias, 2)
    ref = S.softplus64(pre).expand(3, -1)
    bar = S.rounded_bar(1, S.absproduct64(A, Bv), bias.abs(), pre.expand(3, -1), 2)
    el, _ = S.ratios(got, ref, bar)
    assert el <= 1.0, el


def test_colsum_cases_cover_the_kernel_unroll_and_the_column_tiles():
    # 4 row phases, 4 chains of stride 4 per thread: 16 rows per unrolled trip; 64 columns per workgroup
    assert {1, 3, 4, 5, 15, 16, 17, 33, 100} == set(S.COLSUM_M) and {1, 63, 64, 65, 130} == set(S.COLSUM_N)
    for M in S.COLSUM_M:
        assert S.colsum_nsplits(M) == (1, 2, 5, M + 1) and S.nonempty_splits(M, M + 1) < M + 1


def test_grad_plan_offsets_are_the_models():
    offs, tot = S.grad_plan_offsets()
    assert len(offs) == 8 and offs[0] == 0 and all(o % 64 == 0 for o in offs) and tot % 64 == 0
    sizes = []
    for K, N in S.MLP_DIMS:
        sizes += [N * K, N]
    assert all(offs[i] + sizes[i] <= (offs[i + 1] if i < 7 else tot) for i in range(8))
