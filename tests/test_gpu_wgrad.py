"""Kernel-level tests of the WEIGHT-GRADIENT launches, ONE LAUNCH AT A TIME, in every arithmetic of the train step.

`tsr_conv2d_wgrad` / `tsr_conv2d_wgrad_bf16s` are the weight (and bias) gradient of every 1x1 / 3x3 / 5x5 convolution of the
train step.  Each test drives one launch on NaN-surrounded operands into NaN-filled slabs, reduces the partials with
`tsr_reduce_splits` and compares dW and db with fp64 torch autograd on the CPU (tests/_wgrad_check.py: the global bar and the
slice-wise one).

Arithmetics, `planes`, kernels (T = wgrad_mfma_tr16.hip, B = wgrad_b16k.hip):

    f32      -   tsr_conv2d_wgrad: wgrad_mfma_f32_kernel<KS>, 64 x 64 x one kernel row per workgroup, 8 x 8 patches
    bf16x6   3   T wgrad_tr16_kernel<KS, 1, CO, 64, 32, NS = 3>: big 128 x 64 if C_out % 128 == 0, else small 64 x 64
    fp16x3  -2   T wgrad_k32_kernel      \\  big / small per kernel size (one-/two-plane forms, WgradTCfg<KS, 2>):
    bf16op   1   T wgrad_tr16_kernel NS=1  >   3x3: big 128 x 64 x all rows if C_out % 128 == 0, else small 64 x 64 x all rows
    bf16    -1   T ... IO16 or B         /    5x5: big 128 x 128 x 1 row if C_out % 128 == 0 and C_in % 128 == 0, else small
                                              64 x 64 x 2 rows (row groups {0,1}, {2,3}, {4});  1x1: big 128 x 128 on the same
                                              condition, else small 64 x 64
    bf16 (planes -1, bf16 CB16 tensors) picks its kernel by the input: a 3x3 / 5x5 launch WITHOUT an input transform and every
    1x1 launch with C_out = 64 and C_in % 256 == 0 run on B (LDS-DMA; tiles as above; the 1x1 is one 64 x 256 workgroup per 256
    input channels, the virtual form transforms in LDS: "XF"); everything else on T with IO16.  The train engine never hands a
    virtual 3x3 / 5x5 input to the launch: where tsr_conv2d_wgrad_b16k(cout, cin, ks) is 1 it materialises the input with
    tsr_bn_relu_b16 and launches plain.  Every bf16 case with a virtual 3x3 / 5x5 input therefore runs BOTH routes here:
    "direct" (T, IO16) and "materialised" (tsr_bn_relu_b16, then B).

All 16-bit kernels walk (image, 4-row x 8-column patch) work items, f32 walks (image, 8 x 8 patch); split s owns the contiguous
item range [s * per, (s + 1) * per), per = ceil(items / nsplit).  A split whose range is empty -- nsplit above the item count,
or a per that leaves the last splits without items -- still WRITES its partial: exact zeros (include/tactilesr_hip.h says so);
the tests assert that for every empty split of every case, in every arithmetic.

Cases (C_in -> C_out; `virtual` = the input is relu(z * scale + shift) of the stored z; offsets = channel offset of `a`, `dz`
inside buffers 48 channels wider than the slice; everything outside the slices is NaN; slabs are NaN with 8 guard elements):

   #  conv          B  image    input    bias ns  offsets | why
   1  3x3  64-> 64  3  40x40    plain    yes   3  16, 32  | network shape
   2  5x5  64-> 64  2  40x40    virtual  yes   2  32, 16  | network shape; three row groups, the last one short
   3  3x3 128->128  2  13x21    virtual  yes   7  16, 16  | ragged on both axes; 24 items (f32: 12), per = 4 (2): the last split
                                                          | has no item -- exact zeros, not stale NaN
   4  5x5 128->128  5  16x24    plain    NO    5  32, 32  | bias_slab = NULL; 128 x 128 tile, five row groups
   5  1x1 256-> 64  3   9x17    virtual  yes   4  16, 32  | `confusion`; 27 items over 4 splits
   6  3x3 448->128  1  40x40    plain    NO    9  32, 16  | B = 1; widest C_in the network issues (7 C_in tiles); 50 items / 9
   7  5x5  64->128  1   5x3     plain    yes   5   0, 48  | 2 items (f32: 1) < 5 splits: the extra splits hold exact zeros
   8  3x3 192-> 64  2   1x1     virtual  yes   2  16, 32  | image smaller than a patch and than the halo: only the centre tap
                                                          | is non-zero, every other tap slice must be EXACTLY zero; 3 C_in blocks
   9  1x1 128->128 70  12x12    plain    yes  11  32, 16  | 420 items (f32: 280), per = 39 (26): split boundaries inside images
  10  5x5 192->128  2   9x17    virtual  yes   3  16, 16  | C_out 128 with C_in % 128 != 0: small tile, 2 x 3 channel tiles
  11  3x3  64->128  4 100x100   plain    yes   *  32, 32  | Seqs image size; * = the split count the engine would use:
                                                          | tsr_conv2d_wgrad_splits (bf16x6 85, other 16-bit 256), f32: 256
  12p 1x1 512-> 64  2  40x40    plain    yes   3  16, 32  | the C_in % 256 == 0 streaming 1x1 of B, two workgroups per split
  12v 1x1 512-> 64  2  40x40    virtual  yes   3  32, 16  | the same, input transform in LDS (XF)
  13  1x1 192-> 64  3   9x17    virtual  yes   4  16, 32  | ADDED: the only 1x1 that reaches T's SMALL IO16 tile (C_in % 256 != 0)
  14  5x5 128->128  1   6x11    virtual  yes   2  32, 16  | ADDED: the only virtual 5x5 with a 128 x 128 tile (T's BIG IO16 5x5)

Which case runs which instantiation (big | small tile):

    ks  bf16x6 (3)        fp16x3 (-2), bf16op (1)   bf16 (-1) on T, IO16          bf16 (-1) on B
    1   9 | 5 12 13       9 | 5 12 13                9 | 13                        64 x 256: 12p (plain); XF: 5, 12v
    3   3 6 11 | 1 8      3 6 11 | 1 8               3 direct | 8 direct           128 x 64: 3 mat., 6, 11 | 64 x 64: 1, 8 mat.
    5   4 7 10 14 | 2     4 14 | 2 7 10              14 direct | 2 10 direct       128 x 128: 4, 14 mat. | 64 x 64 x 2: 2, 10 mat., 7
    f32: one instantiation per kernel size; 1x1: 5 9 12 13, 3x3: 1 3 6 8 11, 5x5: 2 4 7 10 14.

References (fp64 F.conv2d + autograd.grad on the CPU, cached per case so that the arithmetics share them):
    f32 / bf16x6 / fp16x3   the fp32 operands (a virtual input formed as relu(fma(z, scale, shift)) in fp32);
    bf16op                  the bf16-ROUNDED operands: bf16(a) -- rounded after the fp32 transform, as the kernel does -- and
                            bf16(dz); the tensors handed to the launch are the unrounded fp32 ones, so the kernel's own
                            rounding is part of what is tested;
    bf16                    the stored tensors are bf16(z), bf16(dz); a = bf16(relu(fma(z16, scale, shift))).
    db = sum over (batch, pixels) of the dz tensor AS HANDED TO THE LAUNCH, in fp64: the bias sum does not pass through the
    matrix cores, and bf16op accumulates the fp32 dz it was given (the bf16 arithmetic sums its bf16 tensor).

Bars: dW and db global max-norm relative to the reference's maximum < 1e-5 in all five arithmetics (products of bf16 values
are exact in fp32, so against rounded operands only fp32 summation order is left); dW also slice-wise, every
[64 C_out][64 C_in][kh][kw] slice against its own maximum < max(1e-5, 4 x e_ref), e_ref = the slice-wise error of torch's
fp32 CPU autograd against the same reference (see tests/_wgrad_check.py).  No case is skipped or relaxed for any arithmetic.

Worst figures on an MI355X: NOT RECORDED YET.  Every test prints its figures (`[wgrad summary] case N arith: worst slice
ratio r, global e`, r = slice error as a share of its bar); the table of the worst r and e per arithmetic belongs here and is
to be filled from the first run of this file on the hardware.  What is known from the CPU: e_ref, torch's own fp32 slice
error, is 2.7e-8 (case 8) .. 2.5e-6 (case 4) over the cases, so the bar of every slice but the worst of case 4 is the 1e-5 floor.
"""
import pytest
import torch
import torch.nn.functional as F

import _wgrad_check as WC

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 8
ARITHS = {"f32": None, "bf16x6": 3, "fp16x3": -2, "bf16op": 1, "bf16": -1}

# id: (ks, cin, cout, B, H, W, virtual, bias, ns, a_coff, dz_coff);  ns None = the engine's own split count
CASES = {
    "1": (3, 64, 64, 3, 40, 40, False, True, 3, 16, 32),
    "2": (5, 64, 64, 2, 40, 40, True, True, 2, 32, 16),
    "3": (3, 128, 128, 2, 13, 21, True, True, 7, 16, 16),
    "4": (5, 128, 128, 5, 16, 24, False, False, 5, 32, 32),
    "5": (1, 256, 64, 3, 9, 17, True, True, 4, 16, 32),
    "6": (3, 448, 128, 1, 40, 40, False, False, 9, 32, 16),
    "7": (5, 64, 128, 1, 5, 3, False, True, 5, 0, 48),
    "8": (3, 192, 64, 2, 1, 1, True, True, 2, 16, 32),
    "9": (1, 128, 128, 70, 12, 12, False, True, 11, 32, 16),
    "10": (5, 192, 128, 2, 9, 17, True, True, 3, 16, 16),
    "11": (3, 64, 128, 4, 100, 100, False, True, None, 32, 32),
    "12p": (1, 512, 64, 2, 40, 40, False, True, 3, 16, 32),
    "12v": (1, 512, 64, 2, 40, 40, True, True, 3, 32, 16),
    "13": (1, 192, 64, 3, 9, 17, True, True, 4, 16, 32),
    "14": (5, 128, 128, 1, 6, 11, True, True, 2, 32, 16),
}
PAD = 48


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd  # noqa: F401
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


# ---------------------------------------------------------------------------------------------------------------- operands
class Operands:
    """One case's tensors on the CPU and its cached fp64 references, keyed by operand mode: "f32" (fp32 operands), "op" (bf16
    operands rounded by the kernel from fp32 tensors), "st" (bf16 tensors)."""

    def __init__(self, ks, z, dz, sc=None, sh=None):
        self.ks, self.z, self.dz, self.sc, self.sh = ks, z, dz, sc, sh
        self._ref = {}

    def stored(self, mode):
        """(z, dz) as handed to the launch."""
        return (WC.q16(self.z), WC.q16(self.dz)) if mode == "st" else (self.z, self.dz)

    def seen(self, mode):
        """(a, dz) as the matrix cores see them, fp32 values."""
        z, dz = self.stored(mode)
        a = F.relu(WC.fma32(z, self.sc, self.sh)) if self.sc is not None else z
        return (a, dz) if mode == "f32" else (WC.q16(a), WC.q16(dz))

    def ref(self, mode):
        if mode == "st" and self.sc is None:
            mode_dw = "op"                       # plain input: bf16(bf16(x)) = bf16(x), the two bf16 references coincide
        else:
            mode_dw = mode
        if mode_dw not in self._ref:
            a, dz = self.seen(mode_dw)
            self._ref[mode_dw] = WC.reference(a, dz, self.ks)
        r = dict(self._ref[mode_dw])
        r["db"] = self.stored(mode)[1].double().sum(dim=(0, 2, 3))
        return r


_OPS = {}


def case_operands(cid):
    if cid not in _OPS:
        ks, cin, cout, B, H, W, virtual, _, _, _, _ = CASES[cid]
        g = torch.Generator().manual_seed(1000 + sorted(CASES).index(cid))
        z = torch.randn(B, cin, H, W, generator=g)
        dz = torch.randn(B, cout, H, W, generator=g)
        sc = torch.rand(cin, generator=g) + 0.5 if virtual else None
        sh = torch.randn(cin, generator=g) * 0.3 if virtual else None
        _OPS[cid] = Operands(ks, z, dz, sc, sh)
    return _OPS[cid]


def mode_of(arith):
    return {"bf16op": "op", "bf16": "st"}.get(arith, "f32")


def cb16(x, ctot, coff, dtype):
    """NCHW (cpu) -> flat CB16 device buffer [B][ctot/16][H*W][16]; channels outside [coff, coff + C) are NaN."""
    B, C, H, W = x.shape
    buf = torch.full((B, ctot // 16, H * W, 16), NAN, dtype=dtype)
    buf[:, coff // 16:(coff + C) // 16] = x.reshape(B, C // 16, 16, H * W).permute(0, 1, 3, 2).to(dtype)
    return buf.reshape(-1).cuda()


def items(arith, B, H, W):
    """Work items the kernel family of `arith` splits: (image, 8 x 8 patch) for f32, (image, 4 x 8 patch) otherwise."""
    return B * ((H + 7) // 8 if arith == "f32" else (H + 3) // 4) * ((W + 7) // 8)


def engine_splits(arith, ks, cin, cout, B, H, W):
    """The split count the train engine uses for this launch (tactilesr_amd/model/_train.py: TrainEngine._wgrad)."""
    from tactilesr_amd._lib import load
    if arith == "f32":          # TrainEngine._nsplit: 3 workgroups x 256 CUs x 2 resident slots over the channel / row slices
        return max(1, min(items(arith, B, H, W), 1536 // (ks * (cout // 64) * (cin // 64))))
    return load().tsr_conv2d_wgrad_splits(cout, cin, ks, ARITHS[arith], B, H, W)


class Launch:
    """Device buffers of one launch + the call itself; run() returns the library's status."""

    def __init__(self, arith, ops, ns, a_coff, dz_coff, bias=True, amax=None, plain_a=None):
        """plain_a: (flat bf16 device tensor, channels) -- a materialised input replacing the (virtual) one."""
        self.arith, self.ks, self.ns = arith, ops.ks, ns
        z, dz = ops.stored(mode_of(arith))
        self.B, self.cin, self.H, self.W = z.shape
        self.cout = dz.shape[1]
        dt = torch.bfloat16 if arith == "bf16" else torch.float32
        self.a_ctot, self.a_coff, self.dz_ctot, self.dz_coff = self.cin + PAD, a_coff, self.cout + PAD, dz_coff
        self.dz = cb16(dz, self.dz_ctot, dz_coff, dt)
        if plain_a is not None:
            self.a, self.a_ctot, self.a_coff = plain_a, self.cin, 0
            self.sc = self.sh = None
        else:
            self.a = cb16(z, self.a_ctot, a_coff, dt)
            self.sc = ops.sc.cuda() if ops.sc is not None else None
            self.sh = ops.sh.cuda() if ops.sh is not None else None
        self.n = self.cout * self.cin * self.ks * self.ks
        self.slab = torch.full((ns * self.n + GUARD,), NAN, device="cuda")
        self.bslab = torch.full((ns * self.cout + GUARD,), NAN, device="cuda") if bias else None
        if amax is None:        # the device scalars the producers publish in the engine: max|raw a|, max|dz|
            amax = (float(z.abs().max()), float(dz.abs().max()))
        self.amax = torch.tensor(amax, dtype=torch.float32).cuda() if arith == "fp16x3" else None

    def args(self, **over):
        """Argument list of the entry point, with named overrides (argument checks)."""
        from tactilesr_amd._lib import ptr, stream, c_int as I
        v = dict(a=ptr(self.a), a_ctot=self.a_ctot, a_coff=self.a_coff, cin=self.cin, a_scale=ptr(self.sc),
                 a_shift=ptr(self.sh), dz=ptr(self.dz), dz_ctot=self.dz_ctot, dz_coff=self.dz_coff, cout=self.cout, ks=self.ks,
                 planes=ARITHS[self.arith], a_amax=ptr(self.amax[0:1]) if self.amax is not None else None,
                 dz_amax=ptr(self.amax[1:2]) if self.amax is not None else None, slab=ptr(self.slab), bias_slab=ptr(self.bslab),
                 nsplit=self.ns, B=self.B, H=self.H, W=self.W)
        v.update(over)
        head = [v["a"], I(v["a_ctot"]), I(v["a_coff"]), I(v["cin"]), v["a_scale"], v["a_shift"], v["dz"], I(v["dz_ctot"]),
                I(v["dz_coff"]), I(v["cout"]), I(v["ks"])]
        tail = [v["slab"], v["bias_slab"], I(v["nsplit"]), I(v["B"]), I(v["H"]), I(v["W"]), stream()]
        if self.arith == "f32":
            return "tsr_conv2d_wgrad", head + tail
        return "tsr_conv2d_wgrad_bf16s", head + [I(v["planes"]), v["a_amax"], v["dz_amax"]] + tail

    def run(self, **over):
        from tactilesr_amd._lib import load
        name, a = self.args(**over)
        return getattr(load(), name)(*a)

    def reduce(self):
        """(dW, db or None) on the CPU through tsr_reduce_splits."""
        from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_float as Fl, c_longlong as L
        out = torch.full((self.cout, self.cin, self.ks, self.ks), NAN, device="cuda")
        call("tsr_reduce_splits", ptr(self.slab), ptr(out), L(self.n), I(self.ns), Fl(1.0), stream())
        outb = None
        if self.bslab is not None:
            outb = torch.full((self.cout,), NAN, device="cuda")
            call("tsr_reduce_splits", ptr(self.bslab), ptr(outb), L(self.cout), I(self.ns), Fl(1.0), stream())
        torch.cuda.synchronize()
        return out.cpu(), None if outb is None else outb.cpu()

    def check_slabs(self, label):
        """Every partial written (finite), the guards untouched, the partials of empty splits exactly zero."""
        sl, ns = self.slab.cpu(), self.ns
        assert torch.isnan(sl[ns * self.n:]).all(), f"{label}: wrote behind the last split of slab"
        assert torch.isfinite(sl[:ns * self.n]).all(), f"{label}: a partial of slab was not written"
        n_items = items(self.arith, self.B, self.H, self.W)
        per = (n_items + ns - 1) // ns
        empty = [s for s in range(ns) if s * per >= n_items]
        part = sl[:ns * self.n].view(ns, self.n)
        for s in empty:
            assert not part[s].any(), f"{label}: split {s} has no work item, its partial must be exact zeros"
        for s in set(range(ns)) - set(empty):
            assert part[s].any(), f"{label}: split {s} has work items and an all-zero partial"
        if self.bslab is not None:
            bs = self.bslab.cpu()
            assert torch.isnan(bs[ns * self.cout:]).all(), f"{label}: wrote behind the last split of bias_slab"
            assert torch.isfinite(bs[:ns * self.cout]).all(), f"{label}: a partial of bias_slab was not written"
            for s in empty:
                assert not bs[s * self.cout:(s + 1) * self.cout].any(), f"{label}: bias partial of empty split {s}"
        return empty


def materialise(T, launch):
    """The engine's route for a virtual input of the bf16 arithmetic: tsr_bn_relu_b16 once, then a launch without transform."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    L_ = launch
    mat = torch.full((L_.B * L_.cin * L_.H * L_.W,), NAN, dtype=torch.bfloat16, device="cuda")
    call("tsr_bn_relu_b16", ptr(L_.a), I(L_.a_ctot), I(L_.a_coff), I(L_.cin), ptr(L_.sc), ptr(L_.sh), ptr(mat), I(L_.B),
         I(L_.H * L_.W), stream())
    return mat


def routes(T, arith, ops, ns, a_coff, dz_coff, bias=True, amax=None):
    """The launches one (case, arithmetic) stands for: one, or for bf16 with a virtual 3x3 / 5x5 input the direct launch and
    the engine's materialised one."""
    from tactilesr_amd._lib import load
    first = Launch(arith, ops, ns, a_coff, dz_coff, bias, amax)
    out = [("", first)]
    cout, cin = ops.dz.shape[1], ops.z.shape[1]
    if arith == "bf16" and ops.sc is not None and load().tsr_conv2d_wgrad_b16k(cout, cin, ops.ks):
        mat = materialise(T, first)
        want = ops.seen("st")[0]
        got = mat.cpu().float().view(first.B, cin // 16, first.H * first.W, 16).permute(0, 1, 3, 2).reshape(want.shape)
        assert torch.equal(got, want), "tsr_bn_relu_b16 is not bf16(relu(fma(z, scale, shift)))"
        out.append((" materialised", Launch(arith, ops, ns, a_coff, dz_coff, bias, amax, plain_a=mat)))
    return out


def run_and_check(T, label, arith, ops, ns, a_coff, dz_coff, bias=True, amax=None):
    ref = ops.ref(mode_of(arith))
    worst = (0.0, 0.0)
    for tag, launch in routes(T, arith, ops, ns, a_coff, dz_coff, bias, amax):
        lab = f"[wgrad {label} {arith}{tag} ns={ns}]"
        assert launch.run() == 0, lab
        dw, db = launch.reduce()
        empty = launch.check_slabs(lab)
        e, r, _ = WC.check_dw(dw, ref, lab)
        if bias:
            WC.check_db(db, ref["db"], lab)
        worst = (max(worst[0], r), max(worst[1], e))
        print(f"{lab} empty splits {empty}")
    return worst


# ------------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("cid", list(CASES))
def test_wgrad_case(T, cid, arith):
    ks, cin, cout, B, H, W, virtual, bias, ns, a_coff, dz_coff = CASES[cid]
    if ns is None:
        ns = engine_splits(arith, ks, cin, cout, B, H, W)
        assert 1 <= ns <= items(arith, B, H, W)
    if cid == "7":
        assert ns > items(arith, B, H, W)       # more splits than work items: the extra ones hold exact zeros (check_slabs)
    r, e = run_and_check(T, f"case {cid} k{ks} {cin}->{cout} B={B} {H}x{W}", arith, case_operands(cid), ns, a_coff, dz_coff, bias)
    print(f"[wgrad summary] case {cid} {arith}: worst slice ratio {r:.3f}, global {e:.2e}")


# ------------------------------------------------------------------------------------------------------ fp16x3 dynamic range
RANGE_SHAPES = [(3, 128, 128, 2, 13, 21, 3), (5, 64, 64, 2, 16, 24, 2), (1, 256, 64, 3, 9, 17, 4), (5, 128, 128, 1, 6, 11, 2)]


def _range_operands(shape, virtual, max_scale=1.5):
    ks, cin, cout, B, H, W, _ = shape
    g = torch.Generator().manual_seed(77 + ks + cin + cout)
    z = torch.randn(B, cin, H, W, generator=g)
    dz = torch.randn(B, cout, H, W, generator=g) * 1e-4
    dz[0, 0, 0, 0] = 0.37                        # gradient-like range: tiny values and one large outlier
    z[0, 1, min(2, H - 1), min(3, W - 1)] = 41.0
    sc = sh = None
    if virtual:
        sc = torch.rand(cin, generator=g) * (max_scale - 0.5) + 0.5
        sc[1] = max_scale                        # the outlier's channel carries the largest scale
        sh = torch.randn(cin, generator=g) * 0.3
    return Operands(ks, z, dz, sc, sh)


@pytest.mark.parametrize("virtual", [False, True])
@pytest.mark.parametrize("shape", RANGE_SHAPES)
def test_fp16x3_outliers(T, shape, virtual):
    """dz ~ 1e-4 with one 0.37 outlier, one 41.0 outlier in the input: the power-of-two scales are set by the outliers, the
    bulk of both operands sits 12 binades below them and must still come out within both bars."""
    ops = _range_operands(shape, virtual)
    run_and_check(T, f"range k{shape[0]} {shape[1]}->{shape[2]} virtual={virtual}", "fp16x3", ops, shape[6], 16, 32)


@pytest.mark.parametrize("shape", RANGE_SHAPES)
def test_fp16x3_transform_exceeds_published_amax(T, shape):
    """A virtual input whose scale reaches 8: relu(z * scale + shift) is up to 8 x 41 + shift while the published a_amax is
    that of the RAW z (41).  The kernel must bound the transformed tensor itself: finite and within the bars."""
    ops = _range_operands(shape, True, max_scale=8.0)
    a = ops.seen("f32")[0]
    assert float(a.abs().max()) > 4 * float(ops.z.abs().max())
    run_and_check(T, f"scale8 k{shape[0]} {shape[1]}->{shape[2]}", "fp16x3", ops, shape[6], 32, 16)


@pytest.mark.parametrize("shape", RANGE_SHAPES)
def test_fp16x3_zero_gradient(T, shape):
    """dz identically zero, dz_amax = 0: dW and db are exactly 0 (no 0 * inf from a scale derived from a zero maximum)."""
    ops = _range_operands(shape, True)
    ops.dz.zero_()
    launch = Launch("fp16x3", ops, shape[6], 16, 32, amax=(float(ops.z.abs().max()), 0.0))
    assert launch.run() == 0
    dw, db = launch.reduce()
    assert torch.isnan(launch.slab[launch.ns * launch.n:]).all()
    assert not launch.slab[:launch.ns * launch.n].any() and not dw.any() and not db.any()


# ----------------------------------------------------------------------------------------------------- non-finite propagation
@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("bad", [NAN, float("inf")])
@pytest.mark.parametrize("cid", ["3", "5", "10"])
def test_non_finite_gradient_propagates(T, cid, bad, arith):
    """One NaN / Inf in dz[b, co, y, x]: dW[co] and db[co] are non-finite, as in torch (every tap of every input channel
    multiplies that pixel; Inf * 0 is NaN as well); the published dz_amax is the non-finite maximum the producer's
    atomic max would hold.  In the arithmetics without a data-derived scale every OTHER output channel stays within the bars."""
    ks, cin, cout, B, H, W, _, _, ns, a_coff, dz_coff = CASES[cid]
    base = case_operands(cid)
    ops = Operands(ks, base.z, base.dz.clone(), base.sc, base.sh)
    b, co, y, x = B - 1, 37, H // 2, W // 2                       # interior: every tap pairs the pixel with an in-image input
    ops.dz[b, co, y, x] = bad
    tw = WC.conv_wgrad(ops.seen("f32")[0], ops.dz, ks)          # torch itself
    assert not torch.isfinite(tw[co]).any() and torch.isfinite(tw[torch.arange(cout) != co]).all()
    for tag, launch in routes(T, arith, ops, ns, a_coff, dz_coff, amax=(float(base.z.abs().max()), bad)):
        lab = f"[wgrad non-finite case {cid} {arith}{tag} {bad}]"
        assert launch.run() == 0, lab
        dw, db = launch.reduce()
        assert not torch.isfinite(dw[co]).any(), f"{lab}: finite elements in dW[{co}]"
        assert not torch.isfinite(db[co]), f"{lab}: db[{co}] finite"
        if arith != "fp16x3":
            keep = torch.arange(cout) != co
            assert torch.isfinite(dw[keep]).all() and torch.isfinite(db[keep]).all(), f"{lab}: spread to other output channels"
            ref = base.ref(mode_of(arith))
            clean = dw.clone()
            clean[co] = ref["dw"][co].float()
            WC.check_dw(clean, ref, lab + " other channels")


# ---------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("cid", ["3", "9"])
def test_same_launch_twice_is_bit_identical(T, cid, arith):
    """The header promises deterministic partials (no float atomics): two runs of one launch give the same bits."""
    ks, cin, cout, B, H, W, _, bias, ns, a_coff, dz_coff = CASES[cid]
    for tag, launch in routes(T, arith, case_operands(cid), ns, a_coff, dz_coff, bias):
        assert launch.run() == 0
        torch.cuda.synchronize()
        first, firstb = launch.slab.clone(), launch.bslab.clone()
        launch.slab.fill_(NAN)
        launch.bslab.fill_(NAN)
        assert launch.run() == 0
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int32), launch.slab.view(torch.int32)), f"{arith}{tag}: slab bits differ"
        assert torch.equal(firstb.view(torch.int32), launch.bslab.view(torch.int32)), f"{arith}{tag}: bias_slab bits differ"


# ------------------------------------------------------------------------------------------------------------ argument checks
def _null():
    import ctypes
    return ctypes.c_void_p(0)


BAD_ARGS = {
    "cin = 96": dict(cin=96),
    "a_coff = 8": dict(a_coff=8),
    "a_coff + cin > a_ctot": dict(a_coff=64),
    "ks = 7": dict(ks=7),
    "planes = 2": dict(planes=2),
    "planes = -2 without a_amax": dict(planes=-2, a_amax="null"),
    "a_scale without a_shift": dict(a_shift="null"),
    "nsplit = 0": dict(nsplit=0),
}


def _applies(what, arith):
    if what == "planes = 2":
        return arith != "f32"               # tsr_conv2d_wgrad has no `planes` argument
    if what == "planes = -2 without a_amax":
        return arith == "fp16x3"            # a_amax is required with planes = -2 only
    return True


@pytest.mark.parametrize("what,arith", [(w, a) for w in BAD_ARGS for a in ARITHS if _applies(w, a)])
def test_rejected_call_returns_1_and_writes_nothing(T, what, arith):
    """Each TSR_ERR_ARG branch of both entry points: status 1 before any launch, the NaN-filled slabs stay untouched."""
    over = {k: (_null() if v == "null" else v) for k, v in BAD_ARGS[what].items()}
    ks, cin, cout, B, H, W, _, bias, ns, a_coff, dz_coff = CASES["5"]       # virtual input: a_scale and a_shift are set
    launch = Launch(arith, case_operands("5"), ns, a_coff, dz_coff, bias)
    assert launch.run(**over) == 1, what
    torch.cuda.synchronize()
    assert torch.isnan(launch.slab).all() and torch.isnan(launch.bslab).all(), f"{what}: a rejected call wrote to a slab"
    assert launch.run() == 0                # the same launch without the bad argument is accepted
    torch.cuda.synchronize()
