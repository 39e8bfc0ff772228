"""Case tables, mutation tables, layouts, fp64 references and the per-element checker of tests/test_gpu_infer_b16.py --
everything that runs without a GPU (tests/test_infer_b16_cpu.py checks the argument refusals, the references, the checker and
the tables), plus the pack calls of the bf16-storage inference launches (`tactilesr_amd._lib` is imported inside the
functions that need it, never at module level).

The launches under test are what `conv_impl = "bf16"` runs in eval mode:

    tsr_conv2d_fwd_b16            conv_mfma_split16.hip, one bf16 plane, bf16 tensors; 3x3 / 5x5: 4 images per workgroup, 1x1: 2
    tsr_conv2d_fwd_b16k           conv_b16k.hip B16K_PLAIN: LDS-DMA circular halo, 16x16x32 MFMA, TSR_B16K_NW = 4 images
    tsr_conv2d_fwd_b16k_pair      B16K_PAIR: 17 barrier steps per 32-channel block (9 inner taps + 8 double outer taps), 4 images
    tsr_conv2d_fwd_b16k_fuse1x1   B16K_FUSED: the 64x128 1x1 product in the epilogue, 4 images

Every kernel remaps blockIdx over 8 XCDs (`q = nwg >> 3, r = nwg & 7`); `grid()` below is the launchers' own arithmetic,
ceil(B / images) * ceil(H / 8) * ceil(W / 8).

Every case: input, output and residual slices at three different non-zero channel offsets (16 / 32 / 48, in that order in
`offs`, rotated over the cases) in bf16 CB16 buffers 48 channels wider than the slice (offset 48 = the slice ends the buffer),
NaN everywhere else: a halo row fetched from the wrong channel block, the wrong image or past the image edge reads NaN, not
the zeros that correct padding gives.  Over each table scale / shift take all four NULL combinations and (relu, res) all four.

  B16_CASES (tsr_conv2d_fwd_b16)       scale shift res relu | why                                                    grid
    3x3  64-> 64 B=5  40x40            s  t  res relu       | network shape; 3 absent slots in the last group          50
    1x1 256-> 64 B=3  13x21            s  -  -   -          | unfused `confusion`; 2-image form, last group half empty  12
    5x5  48->128 B=2   5x3             -  t  res -          | odd block count, less than one tile                       1
    3x3  16-> 64 B=1   1x1             -  -  -   relu       | one channel block, image smaller than the halo            1
    3x3 192-> 64 B=1   8x8             s  t  -   -          | fuse-conv width, exactly one tile                         1
    1x1  64->128 B=70 12x12            -  t  res relu       | 35 groups x 4 tiles = 140 workgroups, % 8 == 4          140
    3x3 128-> 64 B=74 12x12            s  -  res -          | 19 groups x 4 tiles = 76 workgroups, % 8 == 4            76
    5x5 128->128 B=6  13x21            -  -  res relu       | ragged on both axes                                      12
    3x3 448-> 64 B=1   8x8             s  -  -   relu       | 28 blocks (a 4032-term sum)                               1

  B16K_CASES (tsr_conv2d_fwd_b16k)
    3x3 128->128 B=5  40x40            s  t  res relu       | network shape                                            50
    5x5 128->128 B=2  13x21            -  -  -   -          | ragged on both axes; B16K_OUT1(.., h), one4 / zero4        6
    3x3  32-> 64 B=1   1x1             s  -  res -          | one channel block, three empty image slots; rb with hs = 1 1
    5x5  96->128 B=3   5x3             -  t  -   relu       | odd block count                                           1
    5x5  64->128 B=1   3x5             s  t  res -          | image smaller than the kernel                             1
    3x3  64-> 64 B=74 12x12            -  t  -   -          | 19 groups x 4 tiles = 76 workgroups, % 8 == 4            76
    3x3 256->128 B=1   8x8             s  -  -   relu       | every slot phase of the 3x3 ring (below)                  1
    5x5 128-> 64 B=9   9x17            -  -  res relu       | every slot phase of the 5x5 ring (below)                 18
  The halo of channel block c lives in physical rows (c * HH + r) & 15, HH = 8 + ks - 1 (B16KGeom).  3x3: HH = 10, the first row
  of block c is 10 c mod 16 = 0, 10, 4, 14, 8, 2, 12, 6 -- period 8 blocks = 256 channels.  5x5: HH = 12, 12 c mod 16 = 0, 12,
  8, 4 -- period 4 blocks = 128 channels.

  PAIR_CASES (tsr_conv2d_fwd_b16k_pair; output in torch.cat([conv3, conv5], 1) order, no permutation)
    C_in  64 B=3  40x40  s t relu   | network shape, one absent slot                                                    25
    C_in  32 B=1   1x1   s - -      | one channel block, image smaller than the halo, three empty slots                   1
    C_in  96 B=5   5x3   - t relu   | odd block count, less than one tile                                                2
    C_in 128 B=3  13x21  - - -      | four blocks, ragged on both axes                                                   6
    C_in  32 B=37  9x17  s - relu   | 10 groups x 6 tiles = 60 workgroups, % 8 == 4                                     60
    C_in 128 B=5   9x17  s t -      |                                                                                   12
    C_in  64 B=1  13x21  - - relu   | B = 1 in a 4-image workgroup                                                       6
    C_in  96 B=3  40x40  - t -      | odd block count at the network's image size                                       25

  FUSE_CASES (tsr_conv2d_fwd_b16k_fuse1x1; (shift2, res, relu2) takes all eight combinations)
    3x3 128 B=2 40x40  relu, s t, (1,1,0) | the model's first launch (w2 = W_a, shift2 = b_c, res = x)                  25
    5x5 128 B=5 40x40  relu, s t, (0,1,1) | the model's second launch (res = P, relu2); 2 groups x 25                   50
    3x3  32 B=1  1x1   -,    s -, (0,0,0) | one channel block, 1x1 image; bq without relu_x2                             1
    5x5  96 B=2  5x3   relu, - t, (1,0,1) | odd block count, less than one tile                                         1
    3x3  96 B=5 13x21  -,    - -, (1,1,1) | odd block count, ragged, one slot of the last group present                 12
    5x5  32 B=1 13x21  relu, s t, (0,0,1) | one channel block, B = 1                                                    6
    3x3 128 B=5  5x3   relu, s t, (1,0,0) |                                                                             2
    5x5 128 B=2  1x1   -,    - t, (0,1,0) | image smaller than the halo                                                 1

Yardstick: fp64 on the bf16-ROUNDED input, residual and weights (fuse1x1: w2 rounded to bf16 and the intermediate rounded to
bf16 once), rounded to bf16 once -- the device differs only by its fp32 accumulation order.  Bar, per element
(`check_elements`): |got - ref| <= max(ulps * 1.01 * 2^-7 |ref|, floor_rel * max|ref_b|), the floor PER IMAGE b, and at least
`min_same` of the elements bit-identical:

    b16, b16k, b16k_pair   ulps 1, floor_rel 3e-6, min_same 0.99      (tests/test_gpu_parity.py test_conv2d_fwd_b16k)
    b16k_fuse1x1           ulps 2, floor_rel 2e-3, min_same 0.98      (test_conv2d_fwd_b16k_fuse1x1)

The only change against those tests is that the floor is taken from the image's maximum, not the tensor's.  Inputs are
randn * 3 per image without outlier and every case asserts max_b max|ref_b| / min_b max|ref_b| < 4 on the CPU, so the per-image
floor is the project's floor up to that factor.  tsr_conv2d_fwd_b16 is held to the b16k bar: the same arithmetic (bf16
operands, fp32 accumulation, one rounding).
"""
import ctypes
from collections import namedtuple

import torch
import torch.nn.functional as F

from _infer_f16s import PAD, NAN, cid, ref_conv, ref_fuse1x1, image_max, image_ratio, he        # noqa: F401  (re-exported)
from test_gpu_conv_ex import cb16, nchw, check_outside_untouched                                  # noqa: F401

BAR = {"b16": (1, 3e-6, 0.99), "b16k": (1, 3e-6, 0.99), "pair": (1, 3e-6, 0.99), "fuse1x1": (2, 2e-3, 0.98)}
NW = 4                                  # TSR_B16K_NW: images per workgroup of every b16k form

B16Case = namedtuple("B16Case", "ks cin cout B H W scale shift res relu offs")
B16_CASES = [
    B16Case(3, 64, 64, 5, 40, 40, True, True, True, 1, (16, 32, 48)),
    B16Case(1, 256, 64, 3, 13, 21, True, False, False, 0, (32, 48, 16)),
    B16Case(5, 48, 128, 2, 5, 3, False, True, True, 0, (48, 16, 32)),
    B16Case(3, 16, 64, 1, 1, 1, False, False, False, 1, (16, 48, 32)),
    B16Case(3, 192, 64, 1, 8, 8, True, True, False, 0, (32, 16, 48)),
    B16Case(1, 64, 128, 70, 12, 12, False, True, True, 1, (48, 32, 16)),
    B16Case(3, 128, 64, 74, 12, 12, True, False, True, 0, (16, 32, 48)),
    B16Case(5, 128, 128, 6, 13, 21, False, False, True, 1, (32, 48, 16)),
    B16Case(3, 448, 64, 1, 8, 8, True, False, False, 1, (48, 16, 32)),
]
B16K_CASES = [
    B16Case(3, 128, 128, 5, 40, 40, True, True, True, 1, (16, 32, 48)),
    B16Case(5, 128, 128, 2, 13, 21, False, False, False, 0, (32, 48, 16)),
    B16Case(3, 32, 64, 1, 1, 1, True, False, True, 0, (48, 16, 32)),
    B16Case(5, 96, 128, 3, 5, 3, False, True, False, 1, (16, 48, 32)),
    B16Case(5, 64, 128, 1, 3, 5, True, True, True, 0, (32, 16, 48)),
    B16Case(3, 64, 64, 74, 12, 12, False, True, False, 0, (48, 32, 16)),
    B16Case(3, 256, 128, 1, 8, 8, True, False, False, 1, (16, 32, 48)),
    B16Case(5, 128, 64, 9, 9, 17, False, False, True, 1, (32, 48, 16)),
]

PairCase = namedtuple("PairCase", "cin B H W scale shift relu offs")
PAIR_CASES = [
    PairCase(64, 3, 40, 40, True, True, 1, (16, 32)),
    PairCase(32, 1, 1, 1, True, False, 0, (32, 48)),
    PairCase(96, 5, 5, 3, False, True, 1, (48, 16)),
    PairCase(128, 3, 13, 21, False, False, 0, (16, 48)),
    PairCase(32, 37, 9, 17, True, False, 1, (32, 16)),
    PairCase(128, 5, 9, 17, True, True, 0, (48, 32)),
    PairCase(64, 1, 13, 21, False, False, 1, (16, 32)),
    PairCase(96, 3, 40, 40, False, True, 0, (32, 48)),
]

FuseCase = namedtuple("FuseCase", "ks cin B H W relu scale shift shift2 res relu2 offs")
FUSE_CASES = [
    FuseCase(3, 128, 2, 40, 40, 1, True, True, True, True, 0, (16, 32, 48)),
    FuseCase(5, 128, 5, 40, 40, 1, True, True, False, True, 1, (32, 48, 16)),
    FuseCase(3, 32, 1, 1, 1, 0, True, False, False, False, 0, (48, 16, 32)),
    FuseCase(5, 96, 2, 5, 3, 1, False, True, True, False, 1, (16, 48, 32)),
    FuseCase(3, 96, 5, 13, 21, 0, False, False, True, True, 1, (32, 16, 48)),
    FuseCase(5, 32, 1, 13, 21, 1, True, True, False, False, 1, (48, 32, 16)),
    FuseCase(3, 128, 5, 5, 3, 1, True, True, True, False, 0, (16, 32, 48)),
    FuseCase(5, 128, 2, 1, 1, 0, False, True, False, True, 0, (32, 48, 16)),
]

TABLES = {"b16": B16_CASES, "b16k": B16K_CASES, "pair": PAIR_CASES, "fuse1x1": FUSE_CASES}


# ---------------------------------------------------------------------------------------------------- launch geometry
def images_per_workgroup(kind, ks=3):
    """launch_b16 (csrc/conv_mfma_split16.hip): 4 for 3x3 / 5x5, 2 for 1x1; b16k_launch (csrc/conv_b16k.hip): TSR_B16K_NW."""
    return 2 if kind == "b16" and ks == 1 else 4


def grid(kind, B, H, W, ks=3):
    img = images_per_workgroup(kind, ks)
    return -(-B // img) * -(-H // 8) * -(-W // 8)


def case_grid(kind, c):
    return grid(kind, c.B, c.H, c.W, getattr(c, "ks", 5))


def ring_rows(ks, cin):
    """First physical halo row of every 32-channel block of a b16k launch: (c * HH) & 15, HH = 8 + ks - 1 (B16KGeom)."""
    return [(c * (8 + ks - 1)) & 15 for c in range(cin // 32)]


def case_slices(kind, c):
    """[(slice width, buffer width, offset)] of every slice the case addresses."""
    if kind in ("b16", "b16k"):
        s = [(c.cin, c.offs[0]), (c.cout, c.offs[1])] + ([(c.cout, c.offs[2])] if c.res else [])
    elif kind == "pair":
        s = [(c.cin, c.offs[0]), (128, c.offs[1])]
    else:
        s = [(c.cin, c.offs[0]), (64, c.offs[1])] + ([(64, c.offs[2])] if c.res else [])
    return [(w, w + PAD, o) for w, o in s]


# ---------------------------------------------------------------------------------------------------- layouts
def slice_buffer_b16(x, coff):
    """NCHW (cpu) -> NaN-filled bf16 CB16 device buffer of C + PAD channels with x at channel offset coff."""
    return cb16(x, x.shape[1] + PAD, coff, torch.bfloat16)


def nan_output_b16(B, c, H, W):
    return torch.full((B * (c + PAD) * H * W,), NAN, dtype=torch.bfloat16, device="cuda")


def read_slice_b16(buf, B, c, H, W, coff):
    """(the slice as fp32 NCHW on the CPU, the whole buffer as NCHW) of a bf16 CB16 device buffer of c + PAD channels; asserts
    that everything outside the slice is still NaN."""
    full = nchw(buf, B, c + PAD, H, W)
    check_outside_untouched(full, coff, c)
    return full[:, coff:coff + c].contiguous(), full


# ---------------------------------------------------------------------------------------------------- fp64 references
def q16(t):
    return None if t is None else t.bfloat16().float()


def round_b16(ref64):
    """The fp64 reference rounded to bf16 once (through fp32, as tests/test_gpu_parity.py does), as fp32 values."""
    return ref64.float().bfloat16().float()


def ref_b16(x, w, scale=None, shift=None, res=None, relu=0):
    """bf16(act(conv(bf16 x, bf16 w) * scale + shift + bf16 res)) with the arithmetic in fp64."""
    return round_b16(ref_conv(q16(x), q16(w), scale, shift, q16(res), relu))


def pair_weight(w3, w5):
    """[128][C_in][5][5]: cat([3x3 weight zero-padded to 5x5, 5x5 weight]) along C_out -- what tsr_pack_conv_weight_b16k_pair takes."""
    return torch.cat([F.pad(w3, (1, 1, 1, 1)), w5], 0).contiguous()


def ref_pair_b16(x, w3, w5, scale=None, shift=None, relu=0):
    """The stage-1 pair in torch.cat order: bf16(act(cat([conv3(x), conv5(x)], 1) * scale + shift))."""
    xq = q16(x).double()
    y = torch.cat([F.conv2d(xq, q16(w3).double(), padding=1), F.conv2d(xq, q16(w5).double(), padding=2)], 1)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    return round_b16(F.relu(y) if relu else y)


def ref_fuse_b16(x, w, scale, shift, relu, w2, shift2=None, res=None, relu2=0):
    """bf16(act2(bf16 w2 . bf16(act(conv(bf16 x, bf16 w) * scale + shift)) + shift2 + bf16 res)), arithmetic in fp64."""
    t = round_b16(ref_conv(q16(x), q16(w), scale, shift, None, relu))
    return round_b16(ref_conv(t, q16(w2).view(64, 128, 1, 1), None, shift2, q16(res), relu2))


# ---------------------------------------------------------------------------------------------------- per-element checker
class ElementMismatch(AssertionError):
    def __init__(self, image, tile, block, what):
        self.image, self.tile, self.block = image, tile, block
        super().__init__(f"{what}: image {image}, 8x8 tile (y {tile[0]}, x {tile[1]}), 16-channel block {block}")


def _where(score):
    b, c, y, x = (int(v) for v in torch.unravel_index(score.argmax(), score.shape))
    return b, (y // 8, x // 8), c // 16


def check_elements(got, ref, ulps, floor_rel, min_same):
    """got, ref: fp32 values of bf16 tensors (NCHW).  Every element within max(ulps * 1.01 * 2^-7 |ref|, floor_rel * max|ref_b|)
    (the floor per image b), at least `min_same` of all elements bit-identical, no non-finite output.  Returns (identical
    share, elements that differ within the bar).  A failure raises ElementMismatch naming the worst (image, 8x8 tile,
    16-channel block): of the largest excess over the bar, or -- for a share below min_same -- the one with the most
    differing elements."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    B = ref.shape[0]
    g, r = got.double(), ref.double()
    d = (g - r).abs()
    bar = torch.maximum(ulps * 1.01 * 2.0 ** -7 * r.abs(), floor_rel * image_max(ref).view(B, 1, 1, 1).expand_as(r))
    fin = torch.isfinite(got)
    if not bool(fin.all()):
        raise ElementMismatch(*_where((~fin).double()), "non-finite output")
    excess = d / bar.clamp_min(1e-300)
    diff = d != 0
    same = 1.0 - float(diff.double().mean())
    if bool((d > bar).any()):
        b, t, k = _where(excess)
        raise ElementMismatch(b, t, k, f"{int((d > bar).sum())} elements beyond the bar (worst {float(excess.max()):.3g} x the bar, "
                                       f"identical share {same:.5f})")
    if same < min_same:
        Bn, C, H, W = ref.shape
        Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
        cnt = F.pad(diff.double(), (0, Wp - W, 0, Hp - H)).view(Bn, C // 16, 16, Hp // 8, 8, Wp // 8, 8).sum(dim=(2, 4, 6))
        b, k, ty, tx = (int(v) for v in torch.unravel_index(cnt.argmax(), cnt.shape))
        raise ElementMismatch(b, (ty, tx), k, f"identical share {same:.5f} below {min_same} (all within the bar)")
    return same, int(diff.sum())


# ---------------------------------------------------------------------------------------------------- inputs
def _vec(g, n, on, kind):
    if not on:
        return None
    return torch.rand(n, generator=g) + 0.5 if kind == "scale" else torch.randn(n, generator=g) * 0.3


def b16_inputs(c, seed=0):
    """CPU operands of one B16Case (None where the case passes NULL)."""
    g = torch.Generator().manual_seed(15000 + seed + c.ks * 7 + c.cin + c.cout + c.B + c.H)
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g) * 3, w=he(g, c.cout, c.cin, c.ks),
                scale=_vec(g, c.cout, c.scale, "scale"), shift=_vec(g, c.cout, c.shift, "shift"),
                res=torch.randn(c.B, c.cout, c.H, c.W, generator=g) if c.res else None, relu=c.relu)


def b16_ref(p):
    return ref_b16(p["x"], p["w"], p["scale"], p["shift"], p["res"], p["relu"])


def pair_inputs(c, seed=0):
    g = torch.Generator().manual_seed(16000 + seed + c.cin + 7 * c.B + c.H)
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g) * 3, w3=he(g, 64, c.cin, 3), w5=he(g, 64, c.cin, 5),
                scale=_vec(g, 128, c.scale, "scale"), shift=_vec(g, 128, c.shift, "shift"), relu=c.relu)


def pair_ref(p):
    return ref_pair_b16(p["x"], p["w3"], p["w5"], p["scale"], p["shift"], p["relu"])


def fuse_inputs(c, seed=0):
    g = torch.Generator().manual_seed(17000 + seed + c.ks * 31 + c.cin + c.B + c.H)
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g) * 3, w=he(g, 128, c.cin, c.ks),
                scale=_vec(g, 128, c.scale, "scale"), shift=_vec(g, 128, c.shift, "shift"), relu=c.relu,
                w2=torch.randn(64, 128, generator=g) * (2.0 / 128) ** 0.5,
                shift2=torch.randn(64, generator=g) * 0.2 if c.shift2 else None,
                res=torch.randn(c.B, 64, c.H, c.W, generator=g) if c.res else None, relu2=c.relu2)


def fuse_ref(p):
    return ref_fuse_b16(p["x"], p["w"], p["scale"], p["shift"], p["relu"], p["w2"], p["shift2"], p["res"], p["relu2"])


INPUTS = {"b16": (b16_inputs, b16_ref), "b16k": (b16_inputs, b16_ref), "pair": (pair_inputs, pair_ref), "fuse1x1": (fuse_inputs, fuse_ref)}


# ---------------------------------------------------------------------------------------------------- entry points
CONV_SIG = ["in:p", "in_ctot:i", "in_coff:i", "cin:i", "w_packed:p", "cout:i", "ks:i", "scale:p", "shift:p", "res:p", "res_ctot:i",
            "res_coff:i", "out:p", "out_ctot:i", "out_coff:i", "relu:i", "B:i", "H:i", "W:i"]
SIGS = {
    "b16": ("tsr_conv2d_fwd_b16", CONV_SIG),
    "b16k": ("tsr_conv2d_fwd_b16k", CONV_SIG),
    "pair": ("tsr_conv2d_fwd_b16k_pair", ["in:p", "in_ctot:i", "in_coff:i", "cin:i", "w_packed:p", "scale:p", "shift:p", "out:p",
                                          "out_ctot:i", "out_coff:i", "relu:i", "B:i", "H:i", "W:i"]),
    "fuse1x1": ("tsr_conv2d_fwd_b16k_fuse1x1", ["in:p", "in_ctot:i", "in_coff:i", "cin:i", "w_packed:p", "ks:i", "scale:p", "shift:p",
                                                "relu:i", "w2_packed:p", "shift2:p", "res:p", "res_ctot:i", "res_coff:i", "out:p",
                                                "out_ctot:i", "out_coff:i", "relu2:i", "B:i", "H:i", "W:i"]),
    "f32": ("tsr_conv2d_fwd", CONV_SIG),
    "bf16s": ("tsr_conv2d_fwd_bf16s", CONV_SIG[:7] + ["nsplit:i"] + CONV_SIG[7:]),
    "pack_f32": ("tsr_pack_conv_weight", ["w:p", "w_packed:p", "cout:i", "cin:i", "ks:i"]),
    "pack_bf16s": ("tsr_pack_conv_weight_bf16s", ["w:p", "w_packed:p", "cout:i", "cin:i", "ks:i", "nsplit:i"]),
    "pack_b16k": ("tsr_pack_conv_weight_b16k", ["w:p", "w_packed:p", "cout:i", "cin:i", "ks:i"]),
    "pack_pair": ("tsr_pack_conv_weight_b16k_pair", ["w:p", "w_packed:p", "cin:i"]),
    "pack_w2": ("tsr_pack_w2_b16k", ["w:p", "w_packed:p"]),
}
FAKE = 16                               # a non-NULL pointer value that is never dereferenced (the CPU test's)


def _cptr(v):
    if v is None:
        return ctypes.c_void_p(0)
    if isinstance(v, int):
        return ctypes.c_void_p(v)
    return ctypes.c_void_p(v.data_ptr())


def raw(kind, vals, stream=None):
    """Status of the entry point of `kind` for the argument list `vals` (name -> tensor / None / fake pointer value / int)."""
    from tactilesr_amd import _lib
    name, sig = SIGS[kind]
    args = []
    for s in sig:
        n, t = s.split(":")
        args.append(_cptr(vals[n]) if t == "p" else ctypes.c_int(vals[n]))
    return getattr(_lib.load(), name)(*args, ctypes.c_void_p(0) if stream is None else stream)


def raw_ex(vals, stream=None):
    """tsr_conv2d_ex on a descriptor filled from `vals` (in / out / res / mask / w_packed pointers as in `raw`)."""
    from tactilesr_amd import _lib
    from tactilesr_amd.model._train import ConvDesc
    d = ConvDesc()
    for k, v in vals.items():
        f = "in_" if k == "in" else k
        v = vals[v] if isinstance(v, str) else v              # ("mask": "res" = the residual's pointer)
        setattr(d, f, _cptr(v).value if dict(ConvDesc._fields_)[f] is ctypes.c_void_p else v)
    return _lib.load().tsr_conv2d_ex(ctypes.byref(d), ctypes.c_void_p(0) if stream is None else stream)


# The valid argument list every refusal test starts from (CPU: fake pointers; GPU: real NaN-padded buffers of these shapes).
REFUSAL_CASES = {
    "b16": B16Case(3, 16, 64, 1, 5, 3, True, True, True, 1, (16, 32, 48)),
    "b16k": B16Case(3, 32, 64, 1, 5, 3, True, True, True, 1, (16, 32, 48)),
    "pair": PairCase(32, 1, 5, 3, True, True, 1, (16, 32)),
    "fuse1x1": FuseCase(3, 32, 1, 5, 3, 1, True, True, True, True, 1, (16, 32, 48)),
    "f32": B16Case(3, 64, 64, 1, 8, 8, True, True, True, 1, (16, 32, 48)),
}
REFUSAL_CASES["bf16s"] = REFUSAL_CASES["ex"] = REFUSAL_CASES["f32"]
OUT_WIDTH = {"pair": 128, "fuse1x1": 64}


def valid_ints(kind):
    """The integer arguments of the valid list of `kind` (pointers are the caller's)."""
    c = REFUSAL_CASES[kind]
    cout = OUT_WIDTH.get(kind) or c.cout
    v = {"in_ctot": c.cin + PAD, "in_coff": c.offs[0], "cin": c.cin, "out_ctot": cout + PAD, "out_coff": c.offs[1], "relu": c.relu,
         "B": c.B, "H": c.H, "W": c.W}
    if kind != "pair":
        v.update(res_ctot=cout + PAD, res_coff=c.offs[2], ks=c.ks)
    if kind == "fuse1x1":
        v.update(relu2=c.relu2)
    if kind not in ("pair", "fuse1x1"):
        v.update(cout=c.cout)
    if kind == "bf16s":
        v.update(nsplit=3)
    if kind == "ex":
        v.update(nsplit=0, epi_mode=0, w_inv_scale=1.0)
    return v


POINTERS = {"b16": ["in", "w_packed", "scale", "shift", "res", "out"], "pair": ["in", "w_packed", "scale", "shift", "out"],
            "fuse1x1": ["in", "w_packed", "scale", "shift", "w2_packed", "shift2", "res", "out"]}
for _k in ("b16k", "f32", "bf16s", "ex"):
    POINTERS[_k] = POINTERS["b16"]
REQUIRED = {"b16": ["in", "w_packed", "out"], "b16k": ["in", "w_packed", "out"], "pair": ["in", "w_packed", "out"],
            "fuse1x1": ["in", "w_packed", "out", "w2_packed"]}


def mutations(kind):
    """[(name, overrides of the valid list)]: every argument list the entry point of `kind` must refuse with status 1."""
    c = REFUSAL_CASES[kind]
    if kind in ("f32", "bf16s", "ex"):            # the negative offsets these three used to accept
        m = [("in_coff negative", {"in_coff": -16}), ("out_coff negative", {"out_coff": -16}), ("res_coff negative", {"res_coff": -16}),
             ("in_coff -cin", {"in_coff": -c.cin}), ("res_coff -cout", {"res_coff": -c.cout})]
        if kind == "ex":
            m.append(("mask_coff negative", {"epi_mode": 2, "mask": "res", "mask_ctot": c.cout + PAD, "mask_coff": -16}))
        return m
    cin, cout, b16k = c.cin, OUT_WIDTH.get(kind) or c.cout, kind != "b16"
    m = [(f"NULL {p}", {p: None}) for p in REQUIRED[kind]]
    m += [(f"{d} = {v}", {d: v}) for d in ("B", "H", "W") for v in (0, -1)]
    m += [("cin = 0", {"cin": 0}), ("cin negative", {"cin": -32 if b16k else -16}), ("cin + 8", {"cin": cin + 8}),
          ("in_ctot - 8", {"in_ctot": cin + PAD - 8}), ("in_coff 8", {"in_coff": 8}), ("out_ctot - 8", {"out_ctot": cout + PAD - 8}),
          ("out_coff 24", {"out_coff": 24}), ("in slice past the end", {"in_coff": PAD + 16}), ("in_coff negative", {"in_coff": -16}),
          ("out slice past the end", {"out_coff": PAD + 16}), ("out_coff negative", {"out_coff": -16}),
          ("in buffer narrower than cin", {"in_ctot": cin - 16, "in_coff": 0}),
          ("out buffer narrower than cout", {"out_ctot": cout - 16, "out_coff": 0})]
    if b16k:
        m += [("cin odd multiple of 16", {"cin": cin + 16}), ("32-bit halo offsets", {"H": 16384, "W": 16384})]
    if kind != "pair":
        m += [("res_ctot - 8", {"res_ctot": cout + PAD - 8}), ("res_coff 8", {"res_coff": 8}), ("res slice past the end", {"res_coff": PAD + 16}),
              ("res_coff negative", {"res_coff": -16}), ("res buffer narrower than cout", {"res_ctot": cout - 16, "res_coff": 0})]
        m += [(f"ks = {v}", {"ks": v}) for v in ((-3, 0, 1, 2, 4, 7) if b16k else (-3, 0, 2, 4, 7))]
    if kind in ("b16", "b16k"):
        m += [(f"cout = {v}", {"cout": v}) for v in (0, 32, 96, 256, -64)]
    return m


def pack_mutations(kind):
    """(valid integer arguments, [(name, overrides)]) of a pack routine (pointers `w`, `w_packed` are the caller's)."""
    null = [("NULL w", {"w": None}), ("NULL w_packed", {"w_packed": None})]
    if kind == "pack_w2":
        return {}, null
    if kind == "pack_pair":
        return {"cin": 32}, null + [("cin = 0", {"cin": 0}), ("cin negative", {"cin": -32}), ("cin 48", {"cin": 48}), ("cin + 8", {"cin": 40})]
    shape = [(f"cout = {v}", {"cout": v}) for v in (0, 32, 96, 256)] + [(f"ks = {v}", {"ks": v}) for v in (-3, 0, 2, 4, 7)]
    if kind == "pack_b16k":
        return ({"cout": 64, "cin": 32, "ks": 3},
                null + shape + [("cin = 0", {"cin": 0}), ("cin negative", {"cin": -32}), ("cin 48", {"cin": 48}), ("cin + 8", {"cin": 40}),
                                ("1x1 with 128 channels", {"ks": 1, "cout": 128})])
    base = {"cout": 64, "cin": 16, "ks": 3}
    if kind == "pack_bf16s":
        base["nsplit"] = 1
    return base, null + shape + [("cin = 0", {"cin": 0}), ("cin negative", {"cin": -16}), ("cin + 8", {"cin": 24})]


# ---------------------------------------------------------------------------------------------------- packs (GPU)
def _L():
    from tactilesr_amd import _lib
    return _lib


def pack_b16(w):
    """tsr_pack_conv_weight_bf16s(nsplit = 1): the weight tsr_conv2d_fwd_b16 takes."""
    L = _L()
    cout, cin, ks, _ = w.shape
    wd = w.cuda().contiguous()
    wp = torch.zeros(L.load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 1), dtype=torch.bfloat16, device="cuda")
    L.call("tsr_pack_conv_weight_bf16s", L.ptr(wd), L.ptr(wp), L.c_int(cout), L.c_int(cin), L.c_int(ks), L.c_int(1), L.stream())
    torch.cuda.synchronize()
    return wp


def pack_b16k(w):
    L = _L()
    cout, cin, ks, _ = w.shape
    wd = w.cuda().contiguous()
    wp = torch.zeros(L.load().tsr_conv_weight_b16k_elems(cout, cin, ks), dtype=torch.bfloat16, device="cuda")
    L.call("tsr_pack_conv_weight_b16k", L.ptr(wd), L.ptr(wp), L.c_int(cout), L.c_int(cin), L.c_int(ks), L.stream())
    torch.cuda.synchronize()
    return wp


def pack_pair_b16k(w3, w5):
    L = _L()
    cin = w3.shape[1]
    wd = pair_weight(w3, w5).cuda()
    wp = torch.zeros(L.load().tsr_conv_weight_b16k_pair_elems(cin), dtype=torch.bfloat16, device="cuda")
    L.call("tsr_pack_conv_weight_b16k_pair", L.ptr(wd), L.ptr(wp), L.c_int(cin), L.stream())
    torch.cuda.synchronize()
    return wp


def pack_w2_b16k(w2):
    L = _L()
    wd = w2.reshape(64, 128).cuda().contiguous()
    wp = torch.zeros(64 * 128, dtype=torch.bfloat16, device="cuda")
    L.call("tsr_pack_w2_b16k", L.ptr(wd), L.ptr(wp), L.stream())
    torch.cuda.synchronize()
    return wp
