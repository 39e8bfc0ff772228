"""Kernel-level tests of the FORWARD boundary launches (csrc/stem_head.hip), ONE LAUNCH AT A TIME: the taxel stem
`tsr_stem_fwd` / `tsr_stem_fwd_b16` and the image head `tsr_head_fwd` / `tsr_head_fwd_b16`.

Every check is one C-ABI launch on NaN-surrounded operands into a NaN-filled output with NaN guard elements behind it,
compared with an fp64 reference on the CPU: `O.bilinear_resize` on the double taxels, `F.conv2d` in double, the affine, the
ReLU.  A channel, an image or a slot the launch must not read holds NaN (a read shows as a NaN result), one it must not
write holds NaN before and after.

Bar: max|y - ref| / max|ref| < 1e-5 per tensor, the project's parity bar, in every case; nothing is relaxed.  The bit-identity
claims (bf16 stem output = the fp32 output rounded to nearest even; untouched images next to a NaN image) come from the
shared kernel template, not from a measurement.

STEM.  The launcher (stem_fwd_impl) picks, per image size, the rows per workgroup RB by an efficiency search over the bands
that fit 32 KB of LDS, and the images per workgroup IPW = clamp(B * bands / 1024, 1, 16).  `stem_plan` below restates that
arithmetic so that each test ASSERTS the path its case is there for; if the launcher's choice changes, the assertion says
which case lost its purpose.  What the launcher gives (H x W, RB, bands, rows of the last band, RB * W mod 16):

    4x4 taxels   sf 1   4x4     RB 4  1 band                       sf 2    8x8    RB 8   1 band
                 sf 3  12x12    RB 4  3 bands                      sf 5   20x20   RB 3   7 bands, last 2, 60 / 40 pixels: 12 / 8
                 sf 8  32x32    RB 2  16 bands                     sf 17  68x68   RB 14  5 bands, last 12, 952 pixels: 8 mod 16
                 sf 31 124x124  RB 16 8 bands, last 12
    3x5  sf 3   9x15  RB 3 (45 pixels: 13 mod 16, W % 4 = 3)       sf 10  30x50  RB 5  (W % 4 = 2)
    1x4  sf 3   3x12  RB 3                                         sf 10  10x40  RB 3, 4 bands, last ONE row
    4x1  sf 3  12x3   RB 12 (W = 3 < 4)                            sf 10  40x10  RB 6, 7 bands, last 4 (W % 4 = 2)
    2x7  sf 3   6x21  RB 3 (63 pixels: 15 mod 16, W % 4 = 1)       sf 10  20x70  RB 10 (W % 4 = 2)
    1x4  sf 1   1x4   and 1x1 sf 1 (1x1): ONE-ROW images, a band of RB = 2 with one live row.  The band search used to start
         at two rows and refused them with status 1; found by this file, fixed in the launcher.
    1x4  sf 169  169x676: RB 2, the widest image whose smallest band fits (see WIDEST below); sf 170 is refused.

    lanes past the last pixel (clamped to pixel npx - 1, masked by `live`): every case whose band pixel count is no multiple
    of 16 above; row pad WP = ((W + 3) & ~3) + 2 with W % 4 = 0, 1, 2, 3.
    IPW > 1 with a tail: sf 1 (one band), B = 2051 -> IPW 2, 1026 workgroups, the last holds ONE image;
                                          B = 16403 -> IPW 16, 1026 workgroups, the last holds THREE images.
    slices: lr_ctot 21 with lr_coff 0 / 3 / 18 (the other 18 taxel channels NaN) x out_ctot 192 with out_coff 0 / 64 / 128.
    epilogue: scale / shift NULL together and one at a time, relu 0 / 1.
    out_amax: max|out| (not max(out)) with an all-negative output; a slot above it is kept, a slot below it raised; NULL.

HEAD, fp32 (head_lds_kernel<false>: 8x8 patches, 16-channel blocks double-buffered in LDS, XCD remap of blockIdx.x):
    cin 16 (nblk = 1: no second buffer), 32 (two blocks: the second load is never followed by a third), 48, 128, 256;
    in_ctot = cin + 64 with NaN behind the slice;
    (B, H, W) -> workgroups: (1,1,1) 1, (2,3,2) 2, (1,8,8) 1: fewer than 8 (qn = 0);  (3,9,17) 18, (7,16,24) 42: not divisible
    by 8 (rn = 2);  (5,7,64) 40: divisible by 8 (rn = 0).

HEAD, bf16 input (tsr_head_fwd_b16): cin 64 / 128 run head_mfma_b16_kernel<2 / 4> on bands of R = 32768 / (36 W) - 2 rows
(capped at H); R < 1 and every other cin run head_lds_kernel<true>:
    (41,40)  R 20: bands of 20, 20 and ONE row          (100,40) R 20: five full bands
    (1,303), (3,303)  R = 1: one / three one-row bands    (2,304)  R = 0: the first width that falls to the LDS form
    (1,1)    R = H = 1
    cin 16 / 32 / 48 / 256 at (9,17): the LDS form on bf16.   in_ctot = cin + 32, NaN behind; relu 0 / 1; B 1 / 3.
    The two forms against each other: one input of width 304, the LDS form on all of it, the MFMA form on its first 303
    columns, H = 3 and H = 2; the outputs agree on columns 0 .. 301 (column 302 sees column 303 in one run only) within
    twice the bar.

Worst figures on an MI355X: NOT RECORDED YET -- this file has not run on the hardware.  Every test prints its figure
(`[stem ...]` / `[head ...]` lines); the worst per group belongs here from the first run.  What is known from the CPU:
torch's own fp32 result is 4e-8 .. 3e-7 from the fp64 reference over these cases, so the 1e-5 bar has room; and the whole
file passes against a torch fp32 restatement of the four launches (layouts, slices, guards, NaN mask, amax logic).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64
TOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _device():
    import tactilesr_amd  # noqa: F401
    from tactilesr_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()


def relerr(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _null():
    return ctypes.c_void_p(0)


# =================================================================================================================== stem
def stem_plan(hin, win, sf, B):
    """stem_fwd_impl's own arithmetic (csrc/stem_head.hip): None where it returns status 1 for lack of LDS."""
    H, W = hin * sf, win * sf
    WP = ((W + 3) & ~3) + 2
    fixed = ((3 * hin * win + 3) & ~3) * 4
    RB, best = 0, -1.0
    for rb in range(2, max(H, 2) + 1):
        if fixed + 3 * (rb + 2) * WP * 4 > 32 * 1024:
            break
        items = slots = 0
        for y in range(0, H, rb):
            r = min(H - y, rb)
            items += r * W
            slots += (r * W + 63) // 64 * 64
        if items / slots > best + 1e-9:
            best, RB = items / slots, rb
    if RB == 0:
        return None
    bands = (H + RB - 1) // RB
    IPW = max(1, min(16, B * bands // 1024))
    return dict(H=H, W=W, RB=RB, bands=bands, last=H - (bands - 1) * RB, IPW=IPW, wgs=(B + IPW - 1) // IPW, tail=B % IPW)


class StemOps:
    """Taxels (B, lr_ctot, hin, win) with NaN outside channels [lr_coff, lr_coff + 3), weight, affine; the fp64 reference
    BEFORE the ReLU is formed once per operand set."""

    def __init__(self, hin, win, B, lr_ctot=3, lr_coff=0, seed=0, negative=False):
        g = torch.Generator().manual_seed(9000 + seed)
        self.hin, self.win, self.B, self.lr_ctot, self.lr_coff = hin, win, B, lr_ctot, lr_coff
        self.lr = torch.full((B, lr_ctot, hin, win), NAN)
        self.lr[:, lr_coff:lr_coff + 3] = torch.rand(B, 3, hin, win, generator=g) * 8
        self.w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
        self.scale = torch.rand(64, generator=g) + 0.5
        self.shift = torch.randn(64, generator=g) * 0.3
        if negative:                       # taxels > 0, weights < 0, shift < 0: every output is negative
            self.w = -self.w.abs() - 0.01
            self.shift = -self.shift.abs()
        self._pre = {}

    def taxels(self):
        return self.lr[:, self.lr_coff:self.lr_coff + 3]

    def ref(self, sf, scale, shift, relu, images=None):
        key = (sf, scale, shift, None if images is None else tuple(images))
        if key not in self._pre:
            tax = self.taxels().double()
            if images is not None:
                tax = tax[list(images)]
            r = F.conv2d(O.bilinear_resize(tax, (self.hin * sf, self.win * sf)), self.w.double(), padding=1)
            if scale:
                r = r * self.scale.double().view(1, -1, 1, 1)
            if shift:
                r = r + self.shift.double().view(1, -1, 1, 1)
            self._pre[key] = r
        return F.relu(self._pre[key]) if relu else self._pre[key]


class Stem:
    """Device buffers of one stem launch and the call; run() returns the library's status."""

    def __init__(self, ops, sf, relu, scale=True, shift=True, out_ctot=64, out_coff=0, b16=False, amax=None):
        self.ops, self.sf, self.relu, self.b16 = ops, sf, relu, b16
        self.out_ctot, self.out_coff = out_ctot, out_coff
        self.H, self.W = ops.hin * sf, ops.win * sf
        self.lr, self.w = ops.lr.cuda(), ops.w.cuda()
        self.scale = ops.scale.cuda() if scale else None
        self.shift = ops.shift.cuda() if shift else None
        self.n = ops.B * out_ctot * self.H * self.W
        self.out = torch.full((self.n + GUARD,), NAN, dtype=torch.bfloat16 if b16 else torch.float32, device="cuda")
        self.amax = None if amax is None else torch.tensor([amax], dtype=torch.float32, device="cuda")

    def run(self, **over):
        from tactilesr_amd._lib import load, ptr, stream, c_int as I
        o = self.ops
        v = dict(lr=ptr(self.lr), lr_ctot=o.lr_ctot, lr_coff=o.lr_coff, axis_cnt=3, hin=o.hin, win=o.win, sf=self.sf,
                 w=ptr(self.w), scale=ptr(self.scale), shift=ptr(self.shift), out=ptr(self.out), out_ctot=self.out_ctot,
                 out_coff=self.out_coff, relu=self.relu, B=o.B)
        v.update(over)
        a = [v["lr"], I(v["lr_ctot"]), I(v["lr_coff"]), I(v["axis_cnt"]), I(v["hin"]), I(v["win"]), I(v["sf"]), v["w"],
             v["scale"], v["shift"], v["out"], I(v["out_ctot"]), I(v["out_coff"]), I(v["relu"]), I(v["B"])]
        if self.b16:
            return load().tsr_stem_fwd_b16(*a, stream())
        return load().tsr_stem_fwd(*a, ptr(self.amax), stream())

    def launch(self):
        assert self.run() == 0
        torch.cuda.synchronize()
        return self

    def result(self, label):
        """The written slice as (B, 64, H, W) on the CPU, in the storage type; everything else must still be NaN."""
        B, HW = self.ops.B, self.H * self.W
        out = self.out.cpu()
        assert torch.isnan(out[self.n:]).all(), f"{label}: wrote behind the output tensor"
        blocks = out[:self.n].view(B, self.out_ctot // 16, HW, 16)
        b0 = self.out_coff // 16
        keep = torch.ones(self.out_ctot // 16, dtype=torch.bool)
        keep[b0:b0 + 4] = False
        assert torch.isnan(blocks[:, keep]).all(), f"{label}: wrote outside channels [{self.out_coff}, {self.out_coff + 64})"
        return blocks[:, b0:b0 + 4].permute(0, 1, 3, 2).reshape(B, 64, self.H, self.W)


def check_stem(label, ops, sf, relu, scale=True, shift=True, out_ctot=64, out_coff=0):
    st = Stem(ops, sf, relu, scale, shift, out_ctot, out_coff).launch()
    got = st.result(label)
    e = relerr(got, ops.ref(sf, scale, shift, relu))
    print(f"[stem {label}] {e:.2e}")
    assert e < TOL, f"{label}: {e:.3e}"
    return got


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("sf", [1, 2, 3, 5, 8, 17, 31])
def test_stem_scale_factors(sf, relu):
    """4x4 taxels, B = 2: every RB / band split the search produces (table in the module docstring)."""
    p = stem_plan(4, 4, sf, 2)
    want = {1: (4, 1, 4), 2: (8, 1, 8), 3: (4, 3, 4), 5: (3, 7, 2), 8: (2, 16, 2), 17: (14, 5, 12), 31: (16, 8, 12)}[sf]
    assert (p["RB"], p["bands"], p["last"]) == want and p["IPW"] == 1
    check_stem(f"sf{sf} relu{relu}", StemOps(4, 4, 2, seed=sf), sf, relu)


def test_stem_scale_factor_set_reaches_the_ragged_paths():
    """The set above holds a short last band, a band and a last band whose pixel count is no multiple of 16 (masked lanes)."""
    plans = [stem_plan(4, 4, sf, 2) for sf in (1, 2, 3, 5, 8, 17, 31)]
    assert any(p["last"] < p["RB"] for p in plans)
    assert any(p["RB"] * p["W"] % 16 for p in plans) and any(p["last"] * p["W"] % 16 for p in plans)
    assert len({p["RB"] for p in plans}) >= 6 and any(p["bands"] == 1 for p in plans)


GRIDS = [(3, 5, 3), (3, 5, 10), (1, 4, 3), (1, 4, 10), (4, 1, 3), (4, 1, 10), (2, 7, 3), (2, 7, 10), (1, 4, 1), (1, 1, 1)]


@pytest.mark.parametrize("hin,win,sf", GRIDS)
def test_stem_other_taxel_grids(hin, win, sf):
    """hin, win other than 4: W % 4 in {0, 1, 2, 3}, W < 4, a last band of one row, one-row images (H = 1)."""
    p = stem_plan(hin, win, sf, 2)
    assert p is not None
    if (hin, win, sf) == (1, 4, 10):
        assert p["last"] == 1 and p["bands"] == 4
    for relu in (0, 1):
        check_stem(f"{hin}x{win} sf{sf} relu{relu}", StemOps(hin, win, 2, seed=100 + 10 * hin + win), sf, relu)


def test_stem_grid_set_covers_every_row_pad():
    assert {win * sf % 4 for _, win, sf in GRIDS} == {0, 1, 2, 3}


@pytest.mark.parametrize("B,ipw,tail", [(2051, 2, 1), (16403, 16, 3)])
def test_stem_several_images_per_workgroup_with_a_tail(B, ipw, tail):
    """sf 1, one band: IPW > 1 and B % IPW != 0.  Every image is written (finite); the images of the last two workgroups and
    every 97th image are compared with fp64."""
    p = stem_plan(4, 4, 1, B)
    assert (p["IPW"], p["tail"], p["bands"]) == (ipw, tail, 1)
    ops = StemOps(4, 4, B, seed=B)
    assert len({tuple(t.flatten().tolist()) for t in ops.taxels()[:64]}) == 64         # distinct images
    got = Stem(ops, 1, 0).launch().result(f"B{B}")
    assert torch.isfinite(got).all(), "an image was not written"
    images = sorted(set(range(0, B, 97)) | set(range((p["wgs"] - 2) * ipw, B)))
    assert len(images) >= ipw + tail
    ref = ops.ref(1, True, True, 0, images)
    e = relerr(got[images], ref)
    print(f"[stem B{B} IPW{ipw}] {e:.2e}")
    assert e < TOL


@pytest.mark.parametrize("out_coff", [0, 64, 128])
@pytest.mark.parametrize("lr_coff", [0, 3, 18])
def test_stem_slices(lr_coff, out_coff):
    """Taxel channels [lr_coff, lr_coff + 3) of 21 (the rest NaN) into channels [out_coff, out_coff + 64) of 192 (the rest
    and the guard stay NaN); sf 5: seven bands, the last one short."""
    check_stem(f"lr_coff{lr_coff} out_coff{out_coff}", StemOps(4, 4, 2, 21, lr_coff, seed=lr_coff), 5, 1, out_ctot=192,
               out_coff=out_coff)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("scale,shift", [(False, False), (True, False), (False, True)])
def test_stem_epilogue_without_affine(scale, shift, relu):
    check_stem(f"scale{int(scale)} shift{int(shift)} relu{relu}", StemOps(4, 4, 2, seed=7), 3, relu, scale, shift)


# WIDEST: the launcher needs fixed + 3 (rb + 2) WP 4 <= 32768 bytes for rb = 2, fixed = ((3 hin win + 3) & ~3) 4 and
# WP = ((W + 3) & ~3) + 2.  For hin = 1, win = 4: fixed = 48, so 48 WP <= 32720, WP <= 681, ((W + 3) & ~3) <= 679, i.e.
# W <= 676 = 4 x 169.  sf 170 (W = 680, WP = 682: 32784 bytes) is refused.
def test_stem_widest_image_is_accepted_and_correct():
    p = stem_plan(1, 4, 169, 1)
    assert p is not None and p["RB"] == 2 and p["last"] == 1 and stem_plan(1, 4, 170, 1) is None
    check_stem("1x4 sf169", StemOps(1, 4, 1, seed=169), 169, 1)


def test_stem_amax_is_max_abs_and_only_raises_the_slot():
    """relu = 0 and an output that is negative everywhere: the slot receives max|out|, bit for bit; a slot above it is
    left alone, one below it raised; NULL is what every other test of this file passes."""
    ops = StemOps(4, 4, 2, seed=55, negative=True)
    for preset, kept in ((0.0, False), (0.5, False), (2.0, True)):
        probe = Stem(ops, 5, 0, amax=0.0).launch()
        out = probe.result("amax")
        big = float(out.abs().max())
        assert float(out.max()) <= 0.0 and float(out.min()) < -1.0       # the scenario: max(out) is not max|out|
        assert relerr(out, ops.ref(5, True, True, 0)) < TOL
        st = Stem(ops, 5, 0, amax=preset * big).launch()
        slot = float(st.amax.cpu()[0])
        assert slot == (torch.tensor(preset * big, dtype=torch.float32).item() if kept else big), (preset, slot, big)
        assert torch.equal(st.result("amax"), out)


B16_CASES = {
    "slice sf5": (dict(hin=4, win=4, B=2, lr_ctot=21, lr_coff=3, seed=3), 5, dict(out_ctot=192, out_coff=64)),
    "IPW2 tail": (dict(hin=4, win=4, B=2051, seed=2051), 1, {}),
    "2x7 sf3": (dict(hin=2, win=7, B=2, seed=127), 3, {}),
    "sf17": (dict(hin=4, win=4, B=2, seed=17), 17, {}),
}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", list(B16_CASES))
def test_stem_b16_is_the_fp32_output_rounded(case, relu):
    """tsr_stem_fwd_b16 is the same kernel template with a round-to-nearest-even store: bit-equal to .bfloat16() of
    tsr_stem_fwd's output, and NaN everywhere else in its (bf16) buffer."""
    okw, sf, skw = B16_CASES[case]
    ops = StemOps(**okw)
    if case == "IPW2 tail":
        assert stem_plan(4, 4, 1, 2051)["IPW"] == 2
    f32 = Stem(ops, sf, relu, **skw).launch().result(case)
    b16 = Stem(ops, sf, relu, b16=True, **skw).launch().result(case + " b16")
    assert b16.dtype == torch.bfloat16 and torch.isfinite(f32).all()
    assert torch.equal(b16, f32.bfloat16())


def test_stem_nan_taxel_stays_in_its_image():
    """One NaN taxel in image 1 of 3: images 0 and 2 are bit-identical to the clean run, image 1 is NaN exactly where the
    fp64 reference is.  sf is EVEN so that no source coordinate is an integer: at an integer coordinate the reference
    multiplies the next taxel by an exact 0 (0 * NaN = NaN) where fp32 coordinates may land just below and never read it.
    out_amax skips the NaN outputs."""
    sf = 10
    ops = StemOps(4, 4, 3, seed=31)
    clean = Stem(ops, sf, 1).launch().result("clean")
    bad = StemOps(4, 4, 3, seed=31)
    bad.lr[1, 1, 1, 2] = NAN
    st = Stem(bad, sf, 1, amax=0.0).launch()
    got = st.result("nan taxel")
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    ref = bad.ref(sf, True, True, 1)
    mask = torch.isnan(ref[1])
    assert mask.any() and not mask.all() and not torch.isnan(ref[[0, 2]]).any()
    assert torch.equal(torch.isnan(got[1]), mask)
    assert relerr(got[1][~mask], ref[1][~mask]) < TOL
    assert float(st.amax.cpu()[0]) == float(got[~torch.isnan(got)].abs().max())


STEM_BAD = {
    "lr NULL": dict(lr="null"), "w NULL": dict(w="null"), "out NULL": dict(out="null"),
    "B = 0": dict(B=0), "B < 0": dict(B=-1),
    "axis_cnt = 1": dict(axis_cnt=1), "axis_cnt = 4": dict(axis_cnt=4),
    "hin = 0": dict(hin=0), "win = 0": dict(win=0), "sf = 0": dict(sf=0), "sf < 0": dict(sf=-2),
    "out_ctot = 200": dict(out_ctot=200), "out_coff = 8": dict(out_coff=8), "out_coff < 0": dict(out_coff=-16),
    "out_coff + 64 > out_ctot": dict(out_coff=144), "lr_coff + 3 > lr_ctot": dict(lr_coff=19), "lr_coff < 0": dict(lr_coff=-1),
}


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
@pytest.mark.parametrize("what", list(STEM_BAD))
def test_stem_rejected_call_returns_1_and_writes_nothing(what, b16):
    """Every TSR_ERR_ARG branch of stem_fwd_impl: status 1 before any launch, the NaN-filled output stays NaN."""
    over = {k: (_null() if v == "null" else v) for k, v in STEM_BAD[what].items()}
    ops = StemOps(4, 4, 2, 21, 3, seed=1)
    st = Stem(ops, 5, 1, out_ctot=192, out_coff=64, b16=b16)
    assert st.run(**over) == 1, what
    torch.cuda.synchronize()
    assert torch.isnan(st.out).all(), f"{what}: a rejected call wrote to the output"
    assert st.run() == 0                     # the same launch without the bad argument is accepted
    torch.cuda.synchronize()


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
def test_stem_image_too_wide_for_the_lds_is_refused(b16):
    """1x4 taxels at sf 170 (see WIDEST): status 1, nothing written.  The buffers have the full size of that image."""
    assert stem_plan(1, 4, 170, 1) is None and stem_plan(1, 4, 169, 1) is not None
    st = Stem(StemOps(1, 4, 1, seed=170), 170, 1, b16=b16)
    assert st.run() == 1
    torch.cuda.synchronize()
    assert torch.isnan(st.out).all()


# =================================================================================================================== head
def head_input(x, in_ctot, dtype):
    """NCHW (cpu) -> flat CB16 device buffer [B][in_ctot/16][H*W][16]; the channels behind C are NaN."""
    B, C, H, W = x.shape
    buf = torch.full((B, in_ctot // 16, H * W, 16), NAN, dtype=dtype)
    buf[:, :C // 16] = x.reshape(B, C // 16, 16, H * W).permute(0, 1, 3, 2).to(dtype)
    return buf.reshape(-1).cuda()


class HeadOps:
    """Input (bf16-representable when b16), weight and the fp64 convolution before the ReLU."""

    def __init__(self, cin, B, H, W, b16, seed=0):
        g = torch.Generator().manual_seed(7000 + seed + cin + 31 * B + 7 * H + W)
        self.x = torch.randn(B, cin, H, W, generator=g)
        if b16:
            self.x = self.x.bfloat16().float()
        self.w = torch.randn(1, cin, 3, 3, generator=g) * 0.05
        self.b16 = b16
        self._pre = None

    def ref(self, relu):
        if self._pre is None:
            self._pre = F.conv2d(self.x.double(), self.w.double(), padding=1)
        return F.relu(self._pre) if relu else self._pre


_HEAD_OPS = {}


def head_ops(cin, B, H, W, b16):
    key = (cin, B, H, W, b16)
    if key not in _HEAD_OPS:
        _HEAD_OPS[key] = HeadOps(cin, B, H, W, b16)
    return _HEAD_OPS[key]


class Head:
    def __init__(self, ops, relu, pad, x=None):
        x = ops.x if x is None else x
        self.b16, self.relu = ops.b16, relu
        self.B, self.cin, self.H, self.W = x.shape
        self.in_ctot = self.cin + pad
        self.x = head_input(x, self.in_ctot, torch.bfloat16 if ops.b16 else torch.float32)
        self.w = ops.w.cuda()
        self.n = self.B * self.H * self.W
        self.out = torch.full((self.n + GUARD,), NAN, device="cuda")

    def run(self, **over):
        from tactilesr_amd._lib import load, ptr, stream, c_int as I
        v = dict(x=ptr(self.x), in_ctot=self.in_ctot, cin=self.cin, w=ptr(self.w), out=ptr(self.out), relu=self.relu,
                 B=self.B, H=self.H, W=self.W)
        v.update(over)
        fn = load().tsr_head_fwd_b16 if self.b16 else load().tsr_head_fwd
        return fn(v["x"], I(v["in_ctot"]), I(v["cin"]), v["w"], v["out"], I(v["relu"]), I(v["B"]), I(v["H"]), I(v["W"]),
                  stream())

    def result(self, label):
        assert self.run() == 0, label
        torch.cuda.synchronize()
        out = self.out.cpu()
        assert torch.isnan(out[self.n:]).all(), f"{label}: wrote behind the image"
        return out[:self.n].view(self.B, 1, self.H, self.W)


def check_head(label, ops, relu, pad):
    got = Head(ops, relu, pad).result(label)
    e = relerr(got, ops.ref(relu))
    print(f"[head {label}] {e:.2e}")
    assert e < TOL, f"{label}: {e:.3e}"


HEAD_SHAPES = [(1, 1, 1), (2, 3, 2), (1, 8, 8), (3, 9, 17), (5, 7, 64), (7, 16, 24)]


def test_head_shapes_cover_the_xcd_remap():
    wgs = [B * ((H + 7) // 8) * ((W + 7) // 8) for B, H, W in HEAD_SHAPES]
    assert wgs == [1, 2, 1, 18, 40, 42]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("B,H,W", HEAD_SHAPES)
@pytest.mark.parametrize("cin", [16, 32, 48, 128, 256])
def test_head_fwd(cin, B, H, W, relu):
    check_head(f"f32 cin{cin} {B}x{H}x{W} relu{relu}", head_ops(cin, B, H, W, False), relu, 64)


def head_b16_band_rows(H, W):
    """head_mfma_launch's band size; 0 = the LDS form."""
    return max(0, min(H, 32 * 1024 // (W * 36) - 2))


MFMA_SHAPES = {(41, 40): 20, (100, 40): 20, (1, 303): 1, (3, 303): 1, (2, 304): 0, (1, 1): 1}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", list(MFMA_SHAPES))
@pytest.mark.parametrize("cin", [64, 128])
def test_head_fwd_b16_bands(cin, H, W, B, relu):
    """cin 64 / 128: the MFMA form at full, ragged and one-row bands, and the first width it hands to the LDS form."""
    assert head_b16_band_rows(H, W) == MFMA_SHAPES[(H, W)]
    if (H, W) == (41, 40):
        assert [min(20, 41 - y) for y in range(0, 41, 20)] == [20, 20, 1]
    check_head(f"b16 cin{cin} {B}x{H}x{W} relu{relu}", head_ops(cin, B, H, W, True), relu, 32)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cin", [16, 32, 48, 256])
def test_head_fwd_b16_lds_form(cin, B, relu):
    check_head(f"b16 lds cin{cin} {B}x9x17 relu{relu}", head_ops(cin, B, 9, 17, True), relu, 32)


@pytest.mark.parametrize("H", [3, 2])
@pytest.mark.parametrize("cin", [64, 128])
def test_head_b16_forms_agree(cin, H):
    """One bf16 input of width 304: head_lds_kernel<true> on all of it (R = 0), head_mfma_b16_kernel on its first 303
    columns (R = 1).  Output columns 0 .. 301 see the same input in both runs and agree within twice the bar."""
    assert head_b16_band_rows(H, 304) == 0 and head_b16_band_rows(H, 303) == 1
    ops = head_ops(cin, 3, H, 304, True)
    lds = Head(ops, 0, 32).result("lds form")
    mfma = Head(ops, 0, 32, x=ops.x[..., :303].contiguous()).result("mfma form")
    ref = ops.ref(0)[..., :302]
    scale = float(ref.abs().max())
    d = float((lds[..., :302].double() - mfma[..., :302].double()).abs().max()) / scale
    print(f"[head forms cin{cin} H{H}] {d:.2e}")
    assert d < 2 * TOL
    assert relerr(lds[..., :302], ref) < TOL and relerr(mfma[..., :302], ref) < TOL


HEAD_BAD = {
    "in NULL": dict(x="null"), "w NULL": dict(w="null"), "out NULL": dict(out="null"),
    "B = 0": dict(B=0), "B < 0": dict(B=-3),
    "cin = 72": dict(cin=72), "cin = 0": dict(cin=0), "cin < 0": dict(cin=-16),
    "in_ctot = 200": dict(in_ctot=200), "cin > in_ctot": dict(in_ctot=64),
    "H = 0": dict(H=0), "W = 0": dict(W=0), "H < 0": dict(H=-9), "W < 0": dict(W=-17),
}


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
@pytest.mark.parametrize("what", list(HEAD_BAD))
def test_head_rejected_call_returns_1_and_writes_nothing(what, b16):
    """Every TSR_ERR_ARG branch of tsr_head_fwd / tsr_head_fwd_b16, H <= 0 and W <= 0 included: status 1 before any launch."""
    over = {k: (_null() if v == "null" else v) for k, v in HEAD_BAD[what].items()}
    head = Head(head_ops(128, 3, 9, 17, b16), 1, 64)
    assert head.run(**over) == 1, what
    torch.cuda.synchronize()
    assert torch.isnan(head.out).all(), f"{what}: a rejected call wrote to the output"
    head.result(what)                        # the same launch without the bad argument is accepted
