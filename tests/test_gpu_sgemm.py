"""Kernel-level tests of the fp32 MFMA SGEMM family (csrc/sgemm_mfma.hip): every tile height and load path of
sgemm_tile_kernel<BM, AF, BF> at its edges, through tsr_sgemm, tsr_sgemm_masked, tsr_sgemm_splitk, tsr_sgemm_splitk_strided,
and tsr_colsum_splitk.  Tables, layouts, data, references and bars: tests/_sgemm_cases.py (preconditions checked without a GPU
by tests/test_sgemm_cases_cpu.py; which form a row launches is the library's own answer, tsr_sgemm_form).

  exact      integer data: the result EQUALS the fp64 reference, element for element (by value: +0 == -0), for the plain,
             ReLU and masked epilogues, for every split-K partial over its own K range (empty trailing splits: zeros) and
             for tsr_reduce_splits of the slab
  rounded    normal data against fp64: elementwise (K + 2) * 2^-24 * (|A|.|B| + |bias|) and global 2e-6; Softplus with
             4 x the fp32 yardstick's own error added; an epilogue probe C = act(B + bias) over [-110, 90]
  guards     every output lives in a larger buffer of a NaN bit pattern which must be bit-identical afterwards (256 floats
             before, 128 rows' worth and more after, the gap of the strided form); operand pads hold NaN
  contain    a NaN / Inf at element 0 or in the interior of A or B gives exactly the reference's NaN / Inf pattern and
             leaves every other element bit-equal to the clean run (the branch-free loads send out-of-range items to
             element 0 and zero them with a select)
  mask       mask values > 0, < 0, +0, -0, NaN, +Inf, -Inf, FLT_MIN against torch.where(ref > 0, v, 0): a select, so a NaN
             in v under a closed mask is 0.  Denormal mask values are left out on purpose: whether `denormal > 0` holds
             depends on the denormal mode the kernel is compiled with, which the header does not promise.
  alignment  a row launched with pointer offsets of 1..3 floats gives the bits of its aligned twin
  production the twelve launches of the MLP at B in {1, 5, 70, 257} and at the smallest batches at which a dW and layer 2's
             forward take 128-row tiles, with the model's strides and slab pointers at the _GradPlan offsets

Worst observed on an MI355X (printed per case and summed up by the last test with `pytest -s`): dot products 0.54 of the
elementwise bar (row masked-49025x4x3-km-f12802; the dx of the last layer at B = 257, K = 3, 0.52) and 1.6e-6 against the global 2e-6 (layer 3's forward at B = 6017,
K = 1024); Softplus 0.49 of its bar (row sgemm-132x4x1-mm-f6422, bias NULL; the probe 0.24); column sums 0.41 of theirs.
"""
import pytest
import torch

import _sgemm_cases as S
from tactilesr_amd import _lib
from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_longlong as L, c_float as Fl

pytestmark = pytest.mark.gpu

BEFORE = 256                # guard floats in front of every output
INF, NAN = float("inf"), float("nan")


class Guarded:
    """`n` output floats inside a buffer of NAN_BITS: BEFORE floats in front, GUARD_ROWS rows' worth (and 256) behind."""

    def __init__(self, n, row):
        self.n = n
        self.bits = torch.full((BEFORE + n + S.GUARD_ROWS * row + 256,), S.NAN_BITS, dtype=torch.int32, device="cuda")
        self.out = self.bits.view(torch.float32)[BEFORE:BEFORE + n]

    def reset(self):
        self.bits.fill_(S.NAN_BITS)

    def check(self, label, written=None):
        """Guards bit-identical; `written` (bool over the n output floats) marks what the launch may write -- the rest of
        the output range must hold the pattern too."""
        assert bool((self.bits[:BEFORE] == S.NAN_BITS).all()), f"{label}: wrote in front of the output"
        assert bool((self.bits[BEFORE + self.n:] == S.NAN_BITS).all()), f"{label}: wrote behind the output"
        if written is not None:
            rest = self.bits[BEFORE:BEFORE + self.n][~written]
            assert bool((rest == S.NAN_BITS).all()), f"{label}: wrote into a gap"


class Operands:
    """Device copies of A (M,K) and B (K,N) in the row's layouts (NaN pads), uploaded once per data set."""

    def __init__(self, c, A, B):
        self.c = c
        self.a_buf = S.place(A, c.af, c.a_off, c.a_pad).cuda()
        self.b_buf = S.place(B.t(), c.bf, c.b_off, c.b_pad).cuda()
        assert self.a_buf.data_ptr() % 16 == 0 and self.b_buf.data_ptr() % 16 == 0
        self.a, self.b = self.a_buf[c.a_off:], self.b_buf[c.b_off:]

    def poke(self, which, e, k, value):
        """Set A(e,k) or B(k,e); returns the old value."""
        c = self.c
        if which == "A":
            buf, idx = self.a_buf, S.element_index(c.af, c.M, c.K, c.a_pad, c.a_off, e, k)
        else:
            buf, idx = self.b_buf, S.element_index(c.bf, c.N, c.K, c.b_pad, c.b_off, e, k)
        old = float(buf[idx])
        buf[idx] = value
        return old


def split_stride(c):
    return c.M * c.N + (S.STRIDED_GAP if c.entry == "splitk_strided" else 0)


def written_mask(c):
    st = split_stride(c)
    w = torch.zeros(c.nsplit, st, dtype=torch.bool, device="cuda")
    w[:, :c.M * c.N] = True
    return w.view(-1)


def new_output(c):
    return Guarded(c.nsplit * split_stride(c), c.N)


def launch(c, ops, g, bias=None, act=0, mask=None):
    """One launch of the row's entry point into the guarded output; returns the result as (nsplit, M, N) -- a copy."""
    g.reset()
    sa0, sa1, sb0, sb1 = S.strides(c)
    ab = [ptr(ops.a), L(sa0), L(sa1), ptr(ops.b), L(sb0), L(sb1)]
    dims = [I(c.M), I(c.N), I(c.K)]
    if c.entry == "sgemm":
        call("tsr_sgemm", *ab, ptr(bias), ptr(g.out), *dims, I(act), stream())
    elif c.entry == "masked":
        call("tsr_sgemm_masked", *ab, ptr(mask), ptr(g.out), *dims, stream())
    elif c.entry == "splitk":
        call("tsr_sgemm_splitk", *ab, ptr(g.out), *dims, I(c.nsplit), stream())
    else:
        call("tsr_sgemm_splitk_strided", *ab, ptr(g.out), L(split_stride(c)), *dims, I(c.nsplit), stream())
    g.check(S.case_id(c), written_mask(c) if c.entry == "splitk_strided" else None)
    return g.out.view(c.nsplit, split_stride(c))[:, :c.M * c.N].reshape(c.nsplit, c.M, c.N).clone()


def reduce_splits(c, g):
    """tsr_reduce_splits over the slab as the model runs it (one call over the whole stride)."""
    st = split_stride(c)
    out = torch.empty(st, device="cuda")
    call("tsr_reduce_splits", ptr(g.out), ptr(out), L(st), I(c.nsplit), Fl(1.0), stream())
    return out[:c.M * c.N].view(c.M, c.N)


def split_reference(c, A, B, absolute=False):
    """(nsplit, M, N) fp64 on the CPU: every partial over its own K range, zeros for the empty ones."""
    ref = torch.zeros(c.nsplit, c.M, c.N, dtype=torch.float64)
    for s, (k0, k1) in enumerate(S.split_ranges(c.K, c.nsplit)):
        if k0 < k1:
            ref[s] = (S.absproduct64 if absolute else S.product64)(A, B, k0, k1)
    return ref


def equal_by_value(got, ref64):
    return bool((got.double() == ref64.cuda()).all())


def same_bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def note(kind, el, gl):
    w = WORST.setdefault(kind, [0.0, 0.0])
    w[0], w[1] = max(w[0], el), max(w[1], gl)


WORST = {}


# ------------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("c", S.TABLE, ids=S.case_id)
def test_exact_on_integer_data(c):
    A, B, bias = S.int_data(c)
    ops, g = Operands(c, A, B), new_output(c)
    if c.entry == "sgemm":
        ref = S.product64(A, B)
        bd = bias.cuda()
        assert equal_by_value(launch(c, ops, g)[0], ref), "plain, bias NULL"
        assert equal_by_value(launch(c, ops, g, bias=bd)[0], ref + bias.double()), "plain, bias"
        assert equal_by_value(launch(c, ops, g, bias=bd, act=1)[0], (ref + bias.double()).clamp_min(0)), "ReLU"
        assert equal_by_value(launch(c, ops, g, act=1)[0], ref.clamp_min(0)), "ReLU, bias NULL"
    elif c.entry == "masked":
        ref = S.product64(A, B)
        mask = S.mask_data(c)
        want = torch.where(mask > 0, ref, torch.zeros((), dtype=torch.float64))
        assert 0.2 < float((mask > 0).double().mean()) < 0.8
        assert equal_by_value(launch(c, ops, g, mask=mask.cuda())[0], want)
    else:
        ref = split_reference(c, A, B)
        got = launch(c, ops, g)
        ne = S.nonempty_splits(c.K, c.nsplit)
        bad = (got.double() != ref.cuda()).flatten(1).any(1)
        assert not bool(bad.any()), f"partials {bad.nonzero().flatten().tolist()[:8]} of {c.nsplit} ({ne} hold work)"
        assert bool((got[ne:] == 0).all())
        assert equal_by_value(reduce_splits(c, g), S.product64(A, B)), "tsr_reduce_splits of the slab"


# ----------------------------------------------------------------------------------------------------------------- rounded
@pytest.mark.parametrize("c", S.TABLE, ids=S.case_id)
def test_rounded_on_normal_data(c):
    A, B, bias = S.normal_data(c)
    ops, g = Operands(c, A, B), new_output(c)
    name = S.case_id(c)
    if c.entry == "sgemm":
        ref, ab, bd = S.product64(A, B), S.absproduct64(A, B), bias.cuda()
        pre = ref + bias.double()
        for act in (0, 1, 2):
            got = launch(c, ops, g, bias=bd, act=act)[0].cpu()
            el, gl = S.check_rounded(f"{name} act {act}", got, S.epilogue64(pre, act), S.rounded_bar(c.K, ab, bias.abs(), pre, act))
            note("softplus" if act == 2 else "dot", el, gl)
        got = launch(c, ops, g, act=2)[0].cpu()
        note("softplus", *S.check_rounded(f"{name} act 2, bias NULL", got, S.softplus64(ref), S.rounded_bar(c.K, ab, None, ref, 2)))
    elif c.entry == "masked":
        ref, ab, mask = S.product64(A, B), S.absproduct64(A, B), S.mask_data(c)
        got = launch(c, ops, g, mask=mask.cuda())[0].cpu()
        assert bool((got[mask <= 0] == 0).all())
        want = torch.where(mask > 0, ref, torch.zeros((), dtype=torch.float64))
        note("dot", *S.check_rounded(name, got, want, S.dot_bound(c.K, ab)))
    else:
        ref, ab = split_reference(c, A, B), split_reference(c, A, B, absolute=True)
        got = launch(c, ops, g).cpu()
        for s, (k0, k1) in enumerate(S.split_ranges(c.K, c.nsplit)):
            if k0 < k1:
                note("dot", *S.check_rounded(f"{name} partial {s}", got[s], ref[s], S.dot_bound(k1 - k0, ab[s])))
            else:
                assert bool((got[s] == 0).all()), s
        full, fab = S.product64(A, B), S.absproduct64(A, B)
        note("dot", *S.check_rounded(f"{name} reduced", reduce_splits(c, g).cpu(), full, S.dot_bound(c.K, fab)))


@pytest.mark.parametrize("forms", ["kk", "mm", "gg"])
def test_epilogue_probe_over_the_softplus_range(forms):
    """K = 1, A = 1: C = act(B + bias) on a grid of pre-activations over [-110, 90], both sides of the threshold 20."""
    A, Bv, bias = S.probe_inputs()
    c = S._c("sgemm", A.shape[0], Bv.shape[1], 1, forms[0], forms[1], 0)
    ops, g, bd = Operands(c, A, Bv), Guarded(A.shape[0] * Bv.shape[1], Bv.shape[1]), bias.cuda()
    pre = (Bv.double() + bias.double()).expand(c.M, -1)              # exact in fp32 (tests/test_sgemm_cases_cpu.py)
    assert equal_by_value(launch(c, ops, g, bias=bd)[0], pre)
    assert equal_by_value(launch(c, ops, g, bias=bd, act=1)[0], pre.clamp_min(0))
    got = launch(c, ops, g, bias=bd, act=2)[0].cpu()
    assert bool((got[pre > 20] == pre[pre > 20].float()).all())    # above the threshold: the identity
    bar = S.rounded_bar(1, S.absproduct64(A, Bv), bias.abs(), pre, 2)
    note("softplus", *S.check_rounded(f"probe {forms}", got, S.softplus64(pre), bar))
    assert bool((got >= 0).all()) and bool((got[1:] == got[:1]).all())


# ------------------------------------------------------------------------------------------------------------- containment
def expected_with_poison(c, A, B, which, e, k, value):
    """fp64 result(s) with A(e,k) or B(k,e) replaced by a NaN / Inf: (nsplit, M, N); only row / column e of the split that
    holds k changes, and there the poison's product with the other operand's row decides NaN or +-Inf."""
    ref = split_reference(c, A, B) if c.entry.startswith("splitk") else S.product64(A, B).unsqueeze(0)
    s = k // S.splitk_chunk(c.K, c.nsplit) if c.entry.startswith("splitk") else 0
    p = torch.tensor(value, dtype=torch.float64)
    if which == "A":
        ref[s, e, :] = ref[s, e, :] - A[e, k].double() * B[k, :].double() + p * B[k, :].double()
    else:
        ref[s, :, e] = ref[s, :, e] - A[:, k].double() * B[k, e].double() + A[:, k].double() * p
    return ref, s


@pytest.mark.parametrize("c", S.TABLE, ids=S.case_id)
def test_nan_and_inf_stay_in_their_row_or_column(c):
    A, B, _ = S.int_data(c, salt=7)
    ops, g = Operands(c, A, B), new_output(c)
    mask = S.mask_data(c) if c.entry == "masked" else None
    md = None if mask is None else mask.cuda()
    clean = launch(c, ops, g, mask=md)
    assert bool(torch.isfinite(clean).all())
    pokes = [("A", 0, 0, NAN), ("B", 0, 0, NAN), ("A", c.M // 2, c.K // 2, INF), ("B", c.N // 2, c.K // 2, NAN),
             ("A", c.M - 1, c.K - 1, NAN), ("B", c.N - 1, c.K - 1, -INF)]
    for which, e, k, value in pokes:
        old = ops.poke(which, e, k, value)
        got = launch(c, ops, g, mask=md)
        ops.poke(which, e, k, old)
        want, s = expected_with_poison(c, A, B, which, e, k, value)
        if mask is not None:
            want = torch.where(mask > 0, want, torch.zeros((), dtype=torch.float64))
        label = f"{which}({e},{k}) = {value}"
        line_g, line_w = (got[s, e, :], want[s, e, :]) if which == "A" else (got[s, :, e], want[s, :, e])
        line_w = line_w.cuda()
        assert bool((torch.isnan(line_g) == torch.isnan(line_w)).all()), f"{label}: NaN pattern of the poisoned line"
        fin = ~torch.isnan(line_w)
        assert bool((line_g[fin].double() == line_w[fin]).all()), f"{label}: Inf / finite values of the poisoned line"
        keep = torch.ones_like(got, dtype=torch.bool)
        if which == "A":
            keep[s, e, :] = False
        else:
            keep[s, :, e] = False
        assert same_bits(got[keep], clean[keep]), f"{label}: an element outside the poisoned line changed"


MASK_VALUES = [1.5, -2.0, 0.0, -0.0, NAN, INF, -INF, 1.1754943508222875e-38]      # the last: FLT_MIN, the smallest normal


@pytest.mark.parametrize("c", [r for r in S.rows("masked") if r.M * r.N < 1 << 16], ids=S.case_id)
def test_mask_is_a_select_on_the_sign_of_the_stored_activation(c):
    A, B, _ = S.int_data(c, salt=11)
    ops, g = Operands(c, A, B), new_output(c)
    vals = torch.tensor(MASK_VALUES)
    mask = vals[torch.randint(0, len(MASK_VALUES), (c.M, c.N), generator=torch.Generator().manual_seed(S.seed_of(c, 12)))]
    mask[0, 0], mask[c.M - 1, c.N - 1] = NAN, -0.0
    i, k = c.M // 2, c.K // 2
    ops.poke("A", i, k, NAN)                                       # a NaN row in v: 0 wherever the mask is closed
    want = S.product64(A, B)
    want[i, :] = NAN
    want = torch.where(mask > 0, want, torch.zeros((), dtype=torch.float64)).cuda()
    got = launch(c, ops, g, mask=mask.cuda())[0]
    assert bool((mask[i] > 0).any()) and bool((~(mask[i] > 0)).any())
    assert bool((torch.isnan(got) == torch.isnan(want)).all())
    fin = ~torch.isnan(want)
    assert bool((got[fin].double() == want[fin]).all())
    for j, v in enumerate(MASK_VALUES):                            # every value, open or closed as `v > 0` says
        sel = (mask == v) if v == v else torch.isnan(mask)
        if v == 0.0:
            sel = sel & (torch.signbit(mask) == torch.signbit(torch.tensor(v)))
        sel[i, :] = False
        assert bool(sel.any()), v
        gs, ws = got[sel.cuda()].double(), S.product64(A, B)[sel].cuda()
        assert bool((gs == (ws if v > 0 else torch.zeros_like(ws))).all()), v


# --------------------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("c", [r for r in S.TABLE if r.a_off or r.b_off], ids=S.case_id)
def test_pointer_offsets_give_the_bits_of_the_aligned_twin(c):
    twin = c._replace(a_off=0, b_off=0)
    assert S.query_form(_lib.load(), twin) != c.form             # the offset is what sends the row down the scalar path
    A, B, bias = S.int_data(c)
    bd = bias.cuda()
    g = new_output(c)
    got = launch(c, Operands(c, A, B), g, bias=bd)
    ref = launch(twin, Operands(twin, A, B), g, bias=bd)
    assert same_bits(got, ref)
    An, Bn, _ = S.normal_data(c)                                  # rounded data: the same sums to within the dot bound
    got = launch(c, Operands(c, An, Bn), g)[0].cpu()
    ref = launch(twin, Operands(twin, An, Bn), g)[0].cpu()
    assert float(((got - ref).abs() / (2 * S.dot_bound(c.K, S.absproduct64(An, Bn)))).max()) <= 1.0


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("c", [S._c("sgemm", 130, 132, 36, "k", "m", 0), S._c("sgemm", 64, 64, 33, "m", "k", 0),
                               S._c("splitk", 68, 48, 65, "m", "m", 0, ns=3)], ids=S.case_id)
def test_every_pointer_offset_on_either_operand(c, off):
    A, B, _ = S.int_data(c)
    g = new_output(c)
    ref = launch(c, Operands(c, A, B), g)
    for a_off, b_off in ((off, 0), (0, off), (off, off)):
        cc = c._replace(a_off=a_off, b_off=b_off)
        assert same_bits(launch(cc, Operands(cc, A, B), g), ref), (a_off, b_off)
    assert equal_by_value(ref.sum(0), S.product64(A, B))


# ------------------------------------------------------------------------------------------------------------------ colsum
@pytest.mark.parametrize("N", S.COLSUM_N)
def test_colsum_splitk(N):
    worst = 0.0
    for M in S.COLSUM_M:
        gen = torch.Generator().manual_seed(1000 * N + M)
        Yi = torch.randint(-S.INT_LIMIT, S.INT_LIMIT + 1, (M, N), generator=gen).float()
        Yn = torch.randn(M, N, generator=gen)
        st = N + S.COLSUM_PAD
        for ns in S.colsum_nsplits(M):
            g = Guarded(ns * st, N)
            w = torch.zeros(ns, st, dtype=torch.bool, device="cuda")
            w[:, :N] = True
            for Y, exact in ((Yi, True), (Yn, False)):
                g.reset()
                call("tsr_colsum_splitk", ptr(Y.cuda()), ptr(g.out), L(st), I(M), I(N), I(ns), stream())
                g.check(f"colsum {M}x{N} ns {ns}", w.view(-1))                   # columns >= N inside split_stride untouched
                got = g.out.view(ns, st)[:, :N].cpu().double()
                for s, (r0, r1) in enumerate(S.split_ranges(M, ns)):
                    ref = Y[r0:r1].double().sum(0) if r0 < r1 else torch.zeros(N, dtype=torch.float64)
                    if exact or r0 >= r1:
                        assert bool((got[s] == ref).all()), (M, ns, s)
                    else:
                        bar = (r1 - r0) * S.U * Y[r0:r1].abs().double().sum(0)
                        err = (got[s] - ref).abs()
                        assert bool((err <= bar).all()), (M, ns, s, float((err / bar.clamp_min(1e-300)).max()))
                        worst = max(worst, float(torch.where(err > 0, err / bar.clamp_min(1e-300), err).max()))
    print(f"[sgemm] colsum N = {N}: worst {worst:.3f} of the bar rows * 2^-24 * sum|y|")
    WORST["colsum"] = max(WORST.get("colsum", 0.0), worst)


# -------------------------------------------------------------------------------------------------------------- production
def production_batch(tag):
    lib = _lib.load()
    return {"dw128": S.batch_dw_128, "fwd128": S.batch_fwd_128}[tag](lib) if isinstance(tag, str) else tag


@pytest.mark.parametrize("kind", ["exact", "rounded"])
@pytest.mark.parametrize("tag", list(S.PRODUCTION_B) + ["dw128", "fwd128"])
def test_the_twelve_launches_of_the_mlp(tag, kind):
    """fwd, dW (+ db) and dx of the four layers as model/tPSFNet.py issues them: its strides, its split count, the dW / db
    partials of all layers in ONE slab at the _GradPlan offsets, one tsr_reduce_splits over the whole of it.  Every launch
    has operands of its own (the chain of the MLP is the end-to-end tests' business)."""
    B = production_batch(tag)
    offs, tot = S.grad_plan_offsets()
    ns = S.production_nsplit(B)
    data = S.int_data if kind == "exact" else S.normal_data
    slab = Guarded(ns * tot, 256)
    written = torch.zeros(ns, tot, dtype=torch.bool, device="cuda")
    checks = []

    def judge(label, got, ref, K, ab, absbias=None, pre=None, act=0):
        if kind == "exact" and act != 2:
            assert bool((got.double() == ref).all()), f"B = {B} {label}"
        elif label.startswith("db"):               # column sums: rows * 2^-24 * sum|y| alone
            el, _ = S.check_rounded(f"B = {B} {label}", got, ref, K * S.U * ab, global_bar=False)
            WORST["colsum"] = max(WORST.get("colsum", 0.0), el)
        else:
            bar = S.rounded_bar(K, ab, absbias, pre, act) if act == 2 else S.dot_bound(K, ab, absbias)
            note("softplus" if act == 2 else "dot", *S.check_rounded(f"B = {B} {label}", got, ref, bar))

    for name, i, c in S.production_cases(B):
        A, Bm, bias = data(c, salt=B)
        ops = Operands(c, A, Bm)
        sa0, sa1, sb0, sb1 = S.strides(c)
        ab_args = [ptr(ops.a), L(sa0), L(sa1), ptr(ops.b), L(sb0), L(sb1)]
        if name.startswith("fwd"):
            act = 1 if i < 3 else 2
            g = Guarded(c.M * c.N, c.N)
            call("tsr_sgemm", *ab_args, ptr(bias.cuda()), ptr(g.out), I(c.M), I(c.N), I(c.K), I(act), stream())
            g.check(name)
            pre = S.product64(A, Bm) + bias.double()
            judge(name, g.out.view(c.M, c.N).cpu(), S.epilogue64(pre, act), c.K, S.absproduct64(A, Bm), bias.abs(), pre, act)
        elif name.startswith("dx"):
            g = Guarded(c.M * c.N, c.N)
            ref = S.product64(A, Bm)
            if i:
                mask = S.mask_data(c, salt=B)
                call("tsr_sgemm_masked", *ab_args, ptr(mask.cuda()), ptr(g.out), I(c.M), I(c.N), I(c.K), stream())
                ref = torch.where(mask > 0, ref, torch.zeros((), dtype=torch.float64))
            else:
                call("tsr_sgemm", *ab_args, ptr(None), ptr(g.out), I(c.M), I(c.N), I(c.K), I(0), stream())
            g.check(name)
            judge(name, g.out.view(c.M, c.N).cpu(), ref, c.K, S.absproduct64(A, Bm))
        else:
            # dW = dy^T x: A(i,k) = dy[k][i], so A's m-fast buffer IS dy (B, N) row-major, which the db launch sums by column
            ow, ob = offs[2 * i], offs[2 * i + 1]
            call("tsr_sgemm_splitk_strided", *ab_args, ptr(slab.out[ow:]), L(tot), I(c.M), I(c.N), I(c.K), I(ns), stream())
            call("tsr_colsum_splitk", ptr(ops.a), ptr(slab.out[ob:]), L(tot), I(B), I(c.M), I(ns), stream())
            written[:, ow:ow + c.M * c.N] = True
            written[:, ob:ob + c.M] = True
            checks.append((name, i, c, A, Bm))
    slab.check(f"B = {B} slab", written.view(-1))
    out = torch.empty(tot, device="cuda")
    call("tsr_reduce_splits", ptr(slab.out), ptr(out), L(tot), I(ns), Fl(1.0), stream())
    parts, out = slab.out.view(ns, tot).cpu(), out.cpu()
    for name, i, c, A, Bm in checks:
        ow, ob = offs[2 * i], offs[2 * i + 1]
        for s, (k0, k1) in enumerate(S.split_ranges(B, ns)):
            gw, gb = parts[s, ow:ow + c.M * c.N].view(c.M, c.N), parts[s, ob:ob + c.M]
            if k0 >= k1:
                assert bool((gw == 0).all()) and bool((gb == 0).all()), (name, s)
                continue
            judge(f"{name} partial {s}", gw, S.product64(A, Bm, k0, k1), k1 - k0, S.absproduct64(A, Bm, k0, k1))
            judge(f"db{i} partial {s}", gb, A[:, k0:k1].double().sum(1), k1 - k0, A[:, k0:k1].abs().double().sum(1))
        judge(f"{name} reduced", out[ow:ow + c.M * c.N].view(c.M, c.N), S.product64(A, Bm), c.K, S.absproduct64(A, Bm))
        judge(f"db{i} reduced", out[ob:ob + c.M], A.double().sum(1), c.K, A.abs().double().sum(1))


def test_zz_report_the_worst_observed_ratios():
    """Prints what the rounded tests of this module saw (run with -s); nothing to assert beyond the bars they held."""
    for kind, w in sorted(WORST.items()):
        print(f"[sgemm] worst over the module, {kind}: {w}")
    for w in WORST.values():
        assert (w if isinstance(w, float) else w[0]) <= 1.0
