"""Case tables, operand layouts, data builders, references and bars of tests/test_gpu_sgemm.py: the fp32 MFMA SGEMM family of
csrc/sgemm_mfma.hip (tsr_sgemm, tsr_sgemm_masked, tsr_sgemm_splitk, tsr_sgemm_splitk_strided, tsr_colsum_splitk).  Nothing here
touches a device: tests/test_sgemm_cases_cpu.py checks every precondition the GPU tests rely on, and which kernel form a row
launches is the library's own answer (tsr_sgemm_form), never a restatement of the dispatch.

A form is BM*100 + AF*10 + BF: BM the tile height (64 / 128), AF / BF the load path of A / B (0 scalar, 1 16-B loads along k,
2 16-B loads along m / n).  sgemm_tile_kernel has 18 of them.

Operand layouts ("stride forms"), with ld = the leading dimension = extent + pad:
    "k"  k-fast:    A(i,k) = a[i*ld + k],    ld = K + pad      (B: B(k,j) = b[j*ld + k])
    "m"  m/n-fast:  A(i,k) = a[k*ld + i],    ld = M + pad      (B: B(k,j) = b[k*ld + j], ld = N + pad)
    "g"  generic:   A(i,k) = a[2*(i*ld + k)], ld = K + pad     (no unit stride at all)
The operand starts `off` floats (0..3) past a 16-B aligned allocation.  Every float of the allocation that is not an element
(leading-dimension pads, the odd slots of "g", the floats before `off`) holds NaN: one that reached a result would show.

Data and bars:
  (a) integers in [-8, 8] for A, B and the bias: every product and every partial sum is an integer below 2^24, exact in fp32
      in any accumulation order, so the kernel must EQUAL the reference (fp64 matmul of the same integers, itself exact).
  (b) normal data against fp64 under two bars: elementwise |got - ref| <= (K + 2) * 2^-24 * (|A|.|B| + |bias|)_ij -- the
      forward-error bound of an fp32 dot product of K terms in any order plus the bias add -- and the project's global
      max|err| / max|ref| < 2e-6.  For a split-K partial K is the length of its own range; for the tsr_reduce_splits sum of ne
      non-empty partials of chunk c the error is at most (c + ne) * 2^-24 * |A|.|B|, and c + ne <= K + 2 always (c * (ne - 1) < K).
      Softplus (act 2): the activation's own rounding is judged like _adam_ex_cases.check_param judges a parameter: the yardstick
      is torch's fp32 CPU softplus of the fp64 pre-activation rounded to fp32, the bar the dot bound (softplus' <= 1) plus
      4 x the yardstick's own elementwise error against fp64.  That error is taken as no less than half an fp32 ulp of the
      fp64 value (yardstick_error): where the yardstick happens to land within 0.02 ulp, as it does next to a small dot bound
      on the K = 3 rows, four times its error is a bar below one ulp, and the fp32 emulation of the reference itself then sits
      at 1.60 of it (row sgemm-130x64x3-km-f6402, bias NULL) -- a bar that fails the reference alone judges luck, not the
      kernel.

Worst observed ratios against the bars are printed by the GPU tests and recorded in the docstring of tests/test_gpu_sgemm.py;
the fp32 NumPy emulation of the reference (sequential accumulation) stays inside both bars on every row
(tests/test_sgemm_cases_cpu.py).
"""
import zlib
from collections import namedtuple

import numpy as np
import torch

from _tpsf_cases import nonempty_splits, splitk_chunk       # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24             # unit roundoff of fp32
GLOBAL_BAR = 2e-6          # test_sgemm_mfma_strides_activations_and_splitk's bar on max|err| / max|ref|
YARD_FACTOR = 4.0          # _adam_ex_cases.check_param's factor on the fp32 yardstick's own error
INT_LIMIT = 8
EXACT_LIMIT = 2 ** 24
NAN_BITS = 0x7FC0BEEF      # a quiet NaN with a recognisable payload
GUARD_ROWS = 128           # at least this many rows' worth of guard follows every output
ALL_FORMS = [bm * 100 + af * 10 + bf for bm in (64, 128) for af in range(3) for bf in range(3)]
ENTRIES = ("sgemm", "masked", "splitk", "splitk_strided")
STRIDED_GAP = 37           # floats between M*N and split_stride in the strided rows (odd: partials lose 16-B alignment)

# entry, M, N, K, stride form of A / B, pointer offset of A / B in floats, leading-dimension pad of A / B, nsplit, form
Case = namedtuple("Case", "entry M N K af bf a_off b_off a_pad b_pad nsplit form")


def _c(entry, M, N, K, af, bf, form, a_off=0, b_off=0, a_pad=0, b_pad=0, ns=1):
    return Case(entry, M, N, K, af, bf, a_off, b_off, a_pad, b_pad, ns, form)


# The smallest shapes that are ragged in every direction: M and N straddle 1, 63/64/65 and 127/128/129/130; K runs over 1, 2,
# 3, 4, 31, 32, 33, 36, 64, 65, 132 (the MFMA consumes k in pairs).  BM = 128 is what M <= 64 gets, and what M > 64 gets once
# ceil(N/128) * ceil(M/128) * nsplit reaches 384.
TABLE = [
    # ---- tsr_sgemm, 128-row tiles with M <= 64 (the upper half of the tile is empty)
    _c("sgemm", 1, 1, 1, "k", "k", 12800),                      # ragged K
    _c("sgemm", 63, 65, 4, "k", "k", 12811),
    _c("sgemm", 64, 64, 32, "k", "m", 12812),
    _c("sgemm", 64, 128, 36, "m", "k", 12821),
    _c("sgemm", 64, 132, 33, "m", "m", 12822),
    _c("sgemm", 63, 129, 31, "m", "m", 12800),                  # ragged M and N
    _c("sgemm", 64, 64, 64, "k", "k", 12801, a_off=1),          # generic by a pointer offset
    _c("sgemm", 64, 64, 64, "k", "m", 12810, b_off=3),
    _c("sgemm", 60, 68, 65, "m", "g", 12820),                   # generic by the strides
    _c("sgemm", 33, 128, 132, "g", "m", 12802),
    _c("sgemm", 64, 64, 32, "k", "k", 12801, a_pad=1),          # generic by a leading dimension that is no multiple of 4
    _c("sgemm", 64, 64, 32, "k", "m", 12810, b_pad=2),
    _c("sgemm", 64, 64, 32, "k", "m", 12812, a_pad=4, b_pad=4),  # extent + 4 stays on the 16-B path
    _c("sgemm", 64, 64, 32, "m", "k", 12821, a_pad=4, b_pad=4),
    _c("sgemm", 1, 127, 2, "k", "m", 12800),
    _c("sgemm", 3, 4, 3, "m", "m", 12802),
    # ---- tsr_sgemm, 64-row tiles (M > 64, few workgroups)
    _c("sgemm", 65, 63, 3, "k", "m", 6400),
    _c("sgemm", 129, 65, 32, "m", "k", 6401),
    _c("sgemm", 130, 64, 3, "k", "m", 6402),                    # the dx of the last layer: one K step, 3 of 32 k-slots
    _c("sgemm", 127, 129, 36, "k", "m", 6410),
    _c("sgemm", 65, 127, 64, "k", "k", 6411),
    _c("sgemm", 129, 132, 132, "k", "m", 6412),
    _c("sgemm", 128, 1, 31, "m", "k", 6420),
    _c("sgemm", 128, 130, 4, "m", "k", 6421),
    _c("sgemm", 128, 128, 33, "m", "m", 6422),
    _c("sgemm", 132, 4, 1, "m", "m", 6422),
    _c("sgemm", 130, 64, 64, "k", "m", 6402, a_off=2),          # pointer offsets 1..3 next to their aligned twins
    _c("sgemm", 130, 64, 64, "k", "m", 6412),
    _c("sgemm", 128, 128, 32, "m", "k", 6420, b_off=1),
    _c("sgemm", 128, 128, 32, "m", "k", 6421),
    _c("sgemm", 128, 128, 32, "m", "m", 6400, a_off=3, b_off=2),
    _c("sgemm", 128, 128, 32, "m", "m", 6402, a_pad=3),
    _c("sgemm", 128, 128, 32, "m", "m", 6422, a_pad=4, b_pad=4),
    # ---- tsr_sgemm, 128-row tiles with rows in the upper half: M > 128 needs 384 workgroups
    _c("sgemm", 5444, 1025, 36, "m", "k", 12821),
    _c("sgemm", 5441, 1025, 33, "k", "k", 12800),
    _c("sgemm", 49025, 4, 4, "k", "m", 12812),                  # wg128 = 384
    _c("sgemm", 49024, 4, 4, "k", "m", 6412),                   # wg128 = 383
    # ---- tsr_sgemm_masked: the dx forms (k-fast dy x n-fast W), both sides of M = 64 / 65 and of wg128 = 383 / 384
    _c("masked", 64, 132, 3, "k", "m", 12802),
    _c("masked", 65, 132, 3, "k", "m", 6402),
    _c("masked", 63, 128, 36, "k", "m", 12812),
    _c("masked", 129, 64, 32, "k", "m", 6412),
    _c("masked", 130, 65, 33, "k", "m", 6400),
    _c("masked", 5444, 1028, 36, "k", "m", 12812),
    _c("masked", 49025, 4, 3, "k", "m", 12802),
    _c("masked", 49024, 4, 3, "k", "m", 6402),
    # ---- tsr_sgemm_splitk: the dW forms (m-fast dy x n-fast x, K = batch)
    _c("splitk", 1, 1, 1, "k", "k", 12800),
    _c("splitk", 63, 65, 33, "k", "m", 12800, ns=2),            # the second split holds one k
    _c("splitk", 3, 256, 70, "m", "m", 12802, ns=5),            # dW of the last layer
    _c("splitk", 64, 48, 70, "m", "m", 12822, ns=5),
    _c("splitk", 65, 48, 70, "m", "m", 6402, ns=5),
    _c("splitk", 68, 48, 65, "m", "m", 6422, ns=3),
    _c("splitk", 130, 130, 132, "k", "k", 12811, ns=96),        # M > 128 on 128-row tiles; 5 of the 96 splits hold work
    _c("splitk", 132, 132, 65, "m", "m", 12822, ns=96),
    _c("splitk", 68, 4, 36, "m", "m", 6422, ns=383),            # wg128 = 383
    _c("splitk", 68, 4, 36, "m", "m", 12822, ns=384),           # wg128 = 384
    # ---- tsr_sgemm_splitk_strided: the same with a gap between the partials
    _c("splitk_strided", 3, 256, 70, "m", "m", 12802, ns=5),
    _c("splitk_strided", 64, 48, 70, "m", "m", 12822, ns=5),
    _c("splitk_strided", 65, 48, 70, "m", "m", 6402, ns=5),
    _c("splitk_strided", 128, 132, 31, "m", "m", 6422, ns=4),
    _c("splitk_strided", 130, 130, 64, "k", "m", 12810, ns=96),
    _c("splitk_strided", 132, 132, 33, "m", "m", 12822, ns=96),
    _c("splitk_strided", 68, 4, 36, "m", "m", 6422, ns=383),
    _c("splitk_strided", 68, 4, 36, "m", "m", 12822, ns=384),
]


def rows(entry=None):
    return [c for c in TABLE if entry is None or c.entry == entry]


def case_id(c):
    s = f"{c.entry}-{c.M}x{c.N}x{c.K}-{c.af}{c.bf}-f{c.form}"
    if c.nsplit != 1:
        s += f"-s{c.nsplit}"
    if c.a_off or c.b_off:
        s += f"-o{c.a_off}{c.b_off}"
    if c.a_pad or c.b_pad:
        s += f"-p{c.a_pad}{c.b_pad}"
    return s


def seed_of(c, salt=0):
    return zlib.crc32(repr(tuple(c)).encode()) + salt


# --------------------------------------------------------------------------------------------------------------- layouts
def layout(form, extent, K, pad):
    """(floats occupied, stride along the extent (m or n), stride along k) of an extent x K operand."""
    if form == "k":
        ld = K + pad
        return extent * ld, ld, 1
    if form == "m":
        ld = extent + pad
        return K * ld, 1, ld
    assert form == "g", form
    ld = K + pad
    return 2 * extent * ld, 2 * ld, 2


def strides(c):
    """(sa0, sa1, sb0, sb1) as the entry points take them."""
    _, sa0, sa1 = layout(c.af, c.M, c.K, c.a_pad)
    _, sb1, sb0 = layout(c.bf, c.N, c.K, c.b_pad)
    return sa0, sa1, sb0, sb1


def place(mat, form, off, pad):
    """Flat fp32 buffer holding `mat` (extent x K) in the layout, NaN everywhere else; the operand starts at buf[off]."""
    extent, K = mat.shape
    size, se, sk = layout(form, extent, K, pad)
    buf = torch.full((off + size,), float("nan"), dtype=torch.float32)
    buf[off:].as_strided((extent, K), (se, sk)).copy_(mat)
    return buf


def element_index(form, extent, K, pad, off, e, k):
    """Index in the flat buffer of element (e along the extent, k)."""
    _, se, sk = layout(form, extent, K, pad)
    return off + e * se + k * sk


def query_form(lib, c):
    """The library's own answer for the row (allocations are 16-B aligned, so alignment is off % 4 == 0)."""
    sa0, sa1, sb0, sb1 = strides(c)
    return lib.tsr_sgemm_form(sa0, sa1, sb0, sb1, int(c.a_off % 4 == 0), int(c.b_off % 4 == 0), c.M, c.N, c.K, c.nsplit)


def masked_loads(c):
    """(A has out-of-range items, B has) for the row's tile height: the tile overhangs the extent or the K range."""
    bm = c.form // 100
    kr = any((min(c.K, (s + 1) * splitk_chunk(c.K, c.nsplit)) - s * splitk_chunk(c.K, c.nsplit)) % 32
             for s in range(nonempty_splits(c.K, c.nsplit)))
    return bool(c.M % bm or kr), bool(c.N % 128 or kr)


# --------------------------------------------------------------------------------------------------------------- data
def int_data(c, salt=0):
    """A (M,K), B (K,N), bias (N): integers in [-8, 8] as fp32."""
    g = torch.Generator().manual_seed(seed_of(c, salt))
    r = lambda *s: torch.randint(-INT_LIMIT, INT_LIMIT + 1, s, generator=g).float()
    return r(c.M, c.K), r(c.K, c.N), r(c.N)


def normal_data(c, salt=0):
    g = torch.Generator().manual_seed(seed_of(c, salt) + 1)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(c.M, c.K), r(c.K, c.N), r(c.N)


def mask_data(c, salt=0):
    """A stored ReLU output: about half zeros, the rest positive."""
    g = torch.Generator().manual_seed(seed_of(c, salt) + 2)
    return torch.randn(c.M, c.N, generator=g).clamp_min(0)


def exactness_margin(A, B, bias=None):
    """Largest (|A|.|B| + |bias|)_ij: below 2^24 every product and every partial sum in any order is exact in fp32."""
    m = A.abs().double() @ B.abs().double()
    if bias is not None:
        m = m + bias.abs().double()
    return float(m.max())


# --------------------------------------------------------------------------------------------------------------- references
def product64(A, B, k0=0, k1=None):
    return A[:, k0:k1].double() @ B[k0:k1].double()


def absproduct64(A, B, k0=0, k1=None):
    return A[:, k0:k1].abs().double() @ B[k0:k1].abs().double()


def split_ranges(K, nsplit):
    """[(k0, k1)] of every split; empty trailing ranges have k0 >= k1."""
    ch = splitk_chunk(K, nsplit)
    return [(s * ch, min((s + 1) * ch, K)) for s in range(nsplit)]


def softplus64(pre):
    """Softplus(beta 1, threshold 20) in fp64, as the model defines it."""
    return torch.nn.functional.softplus(pre.double())


def softplus_yardstick(pre64):
    return torch.nn.functional.softplus(pre64.float()).double()


def epilogue64(pre, act):
    if act == 1:
        return pre.clamp_min(0)
    if act == 2:
        return softplus64(pre)
    return pre


def dot_bound(K, absprod, absbias=None):
    b = absprod if absbias is None else absprod + absbias.double()
    return (K + 2) * U * b


def half_ulp32(x64):
    """Half a unit in the last place of the fp32 numbers next to |x| (normal range): what rounding x to fp32 may cost."""
    return torch.exp2(torch.floor(torch.log2(x64.abs().clamp_min(2.0 ** -126))) - 24)


def yardstick_error(pre64):
    """|yardstick - fp64| per element, taken as no less than half an ulp of the fp64 value: an element where the yardstick
    happens to land closer than its own format guarantees would set a bar no fp32 result can be asked to meet."""
    sp = softplus64(pre64)
    return torch.maximum((softplus_yardstick(pre64) - sp).abs(), half_ulp32(sp))


def rounded_bar(K, absprod, absbias, pre64, act):
    """Elementwise bar of (b) for act(pre)."""
    bar = dot_bound(K, absprod, absbias)
    if act == 2:
        bar = bar + YARD_FACTOR * yardstick_error(pre64)
    return bar


def ratios(got, ref, bar):
    """(worst |got - ref| / bar over the elements, max|err| / max|ref|); a NaN anywhere gives inf."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf"), float("inf")
    el = torch.where(err > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
    return float(el.max()), float(err.max() / ref.abs().max().clamp_min(1e-30))


def check_rounded(label, got, ref, bar, global_bar=True):
    """Assert both bars (the column sums have the elementwise one only); prints and returns the two figures."""
    el, gl = ratios(got, ref, bar)
    print(f"[sgemm] {label}: {el:.3f} of the elementwise bar, global {gl:.2e} (bar {GLOBAL_BAR:.0e})")
    assert el <= 1.0, (label, el)
    assert gl < GLOBAL_BAR or not global_bar, (label, gl)
    return el, gl


# fp32 emulation of the reference on the CPU: sequential accumulation over k, one rounding per multiply and per add
def emulate32(A, B, bias=None, act=0, k0=0, k1=None):
    a, b = A.numpy().astype(np.float32), B.numpy().astype(np.float32)
    k1 = a.shape[1] if k1 is None else k1
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(k0, k1):
        acc += a[:, k:k + 1] * b[k:k + 1, :]
    if bias is not None:
        acc = acc + bias.numpy().astype(np.float32)
    if act == 1:
        acc = np.maximum(acc, np.float32(0))
    elif act == 2:
        with np.errstate(over="ignore"):
            acc = np.where(acc > np.float32(20), acc, np.log1p(np.exp(acc, dtype=np.float32), dtype=np.float32))
    return torch.from_numpy(acc.astype(np.float32))


# --------------------------------------------------------------------------------------------------------------- epilogue probe
def probe_grid():
    """Pre-activations over [-110, 90]: a coarse grid, a fine one around 0 and points on both sides of the threshold 20."""
    coarse = torch.arange(-110.0, 90.5, 0.5)
    fine = torch.arange(-4.0, 4.0, 1.0 / 64)
    near = 20.0 + torch.tensor([-1.0, -2.0 ** -10, -2.0 ** -18, 0.0, 2.0 ** -18, 2.0 ** -10, 1.0])
    return torch.cat([coarse, fine, near]).float()


def probe_inputs():
    """K = 1, A = 1: C = act(B + bias).  Returns A (M,1), B (1,N), bias (N)."""
    pre = probe_grid()
    bias = torch.tensor([0.0, 0.25, -0.5]).repeat((pre.numel() + 2) // 3)[:pre.numel()]
    return torch.ones(3, 1), (pre - bias).view(1, -1), bias          # B + bias is the grid again, exactly


# --------------------------------------------------------------------------------------------------------------- colsum
COLSUM_M = (1, 3, 4, 5, 15, 16, 17, 33, 100)
COLSUM_N = (1, 63, 64, 65, 130)
COLSUM_PAD = 5             # columns between N and split_stride


def colsum_nsplits(M):
    return (1, 2, 5, M + 1)


# --------------------------------------------------------------------------------------------------------------- production
MLP_DIMS = [(48, 256), (256, 1024), (1024, 256), (256, 3)]      # (in, out) of MLP_layer 1, 3, 5, 7
PRODUCTION_B = (1, 5, 70, 257)


def production_nsplit(B):
    """The split count of the tPSFNet backward (model/tPSFNet.py)."""
    return max(1, min(32, (B + 15) // 16))


def production_cases(B):
    """The twelve launches of the MLP at batch B with the strides model/tPSFNet.py passes: [(name, layer, Case)] with form 0
    (the form is the query's to tell).  fwd: x (B,K) k-fast times W (N,K) k-fast; dW: dy (B,N) read m-fast times x (B,K) read
    n-fast, reduced over the batch in production_nsplit(B) splits into the shared slab; dx: dy (B,N) k-fast times W (N,K)
    n-fast, masked by the layer below (layer 0: plain tsr_sgemm, no bias)."""
    ns = production_nsplit(B)
    out = []
    for i, (K, N) in enumerate(MLP_DIMS):
        out.append((f"fwd{i}", i, _c("sgemm", B, N, K, "k", "k", 0)))
        out.append((f"dW{i}", i, _c("splitk_strided", N, K, B, "m", "m", 0, ns=ns)))
        out.append((f"dx{i}", i, _c("masked" if i else "sgemm", B, K, N, "k", "m", 0)))
    return out


def grad_plan_offsets():
    """(offsets of the eight parameter slots, total) of the flat gradient buffer, from the model's own _GradPlan."""
    from tactilesr_amd.model.tPSFNet import _GradPlan
    params = []
    for K, N in MLP_DIMS:
        params += [torch.empty(N, K), torch.empty(N)]
    plan = _GradPlan(params, torch.device("cpu"))
    return list(plan.offsets), plan.total


def smallest_batch(lib, pred, limit=20000):
    """Smallest B in 1..limit whose production forms (name -> form) satisfy pred, by the library's query."""
    for B in range(1, limit + 1):
        if pred({name: query_form(lib, c) for name, _, c in production_cases(B)}):
            return B
    raise AssertionError("no batch below the limit")


def batch_dw_128(lib):
    """Smallest B at which a dW launch with M > 64 takes 128-row tiles."""
    return smallest_batch(lib, lambda f: any(f[f"dW{i}"] // 100 == 128 for i in range(3)))


def batch_fwd_128(lib):
    """Smallest B at which layer 2's forward (fwd1: the 256 -> 1024 layer) AND a dW take 128-row tiles with M > 64."""
    return smallest_batch(lib, lambda f: f["fwd1"] // 100 == 128 and any(f[f"dW{i}"] // 100 == 128 for i in range(3)))
