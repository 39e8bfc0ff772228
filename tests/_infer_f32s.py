"""Case tables, launch geometry, references, pack restatements and mutation tables of tests/test_gpu_infer_f32s.py --
everything that runs without a GPU (tests/test_infer_f32s_cpu.py checks the tables, the references and the refusals), plus the
pack calls of the fp32 and split-bf16 inference launches (`tactilesr_amd._lib` is imported inside the functions that need it,
never at module level).

The launches under test are the INFERENCE instantiations (`EXT = false`) behind four of the five eval arithmetics:

    arith  entry point                         kernel                                              images per workgroup
    f32    tsr_conv2d_fwd                      conv_mfma_f32.hip, v_mfma_f32_32x32x2_f32           2
    x6     tsr_conv2d_fwd_bf16s, nsplit = 3    conv_mfma_split16.hip, 3 bf16 planes, 6 products    2
    x3     tsr_conv2d_fwd_bf16s, nsplit = 2    2 planes, 3 products                                2
    bf16   tsr_conv2d_fwd_bf16s, nsplit = 1    1 plane (fp32 tensors, not the bf16-storage path)   3x3 / 5x5: 4, 1x1: 2

with weights from tsr_pack_conv_weight (f32) / tsr_pack_conv_weight_bf16s.  The split16 inference instances take their weight
slab by LDS-DMA into a 3-slot ring (`DMA_W` / `DMA_WAIT_N`); a pass over a slab whose 16-byte item count is no multiple of 256
is issued by some of the four waves only.  `instance()` names the template instance a shape runs; there are 28:

    f32          (ks, cout)            ks in {1, 3, 5}, cout in {64, 128}                                         6
    x6, x3       (ks, cout, form)      3x3: "dbh" (double-buffered halo, cin / 16 even) or "single" (odd)         8 each
    bf16         (ks, cout)                                                                                       6

Padded tap slots per channel block (`tap_slots`: steps x taps per step, from the kernel's `taps_per_step`; the tail of the
last step holds zero weight):

    arith  1x1          3x3 cout 64    3x3 cout 128   5x5 cout 64     5x5 cout 128
    x6     1 (1x1)      9 (9x1)        9 (9x1)        25 (25x1)       25 (25x1)
    x3     1 (1x1)      10 (5x2)       10 (5x2)       26 (13x2)       26 (13x2)
    bf16   1 (1x1)      9 (3x3)        9 (3x3)        25 (5x5)        27 (9x3)

16-byte items of one step's weight slab (`slab_items`, cout 64 / 128; a DMA pass moves 256, one wave 64): x6 384 / 768 -- at
cout 64 the second pass comes from waves 0-1 only; x3 512 / 1024 (1x1: 256 / 512); bf16 1x1 128 (two waves issue) / 256, 3x3
384 / 768, 5x5 640 / 768.

1. One launch at a time.  Every case: input, output and residual slices at three different non-zero channel offsets (16 / 32
/ 48, in that order in `offs`, rotated over the cases) in fp32 CB16 buffers 48 channels wider than the slice, NaN everywhere
else; inputs randn * 3 without outlier, `image_ratio(ref) < 4` asserted on the CPU; every output element checked per image
(`check_images`), everything outside the output slice still NaN.  Over each table (scale, shift) take all four NULL
combinations and (res, relu) all four.  The trailing number is the grid, ceil(B / images) * ceil(H / 8) * ceil(W / 8).

  F32_CASES (arith f32)                  scale shift res relu | instance  | why                                          grid
    3x3  64-> 64 B=3  40x40              s t res relu         | (3, 64)   | network shape, absent slot                     50
    5x5 128->128 B=2  13x21              s - -   -            | (5, 128)  | ragged                                          6
    1x1  16-> 64 B=1   1x1               - t res -            | (1, 64)   | S = 1: the `s + 1 < S` prefetch is never taken   1
    1x1  32->128 B=5   9x17              - - -   relu         | (1, 128)  | S = 2, last group half empty                   18
    3x3  16->128 B=1   5x3               s t -   -            | (3, 128)  | one block, less than a tile                     1
    5x5  48-> 64 B=2   1x1               - t res relu         | (5, 64)   | odd block count, image smaller than the halo     1
    5x5  16-> 64 B=1   3x5               s - res -            | (5, 64)   | image smaller than the kernel                    1
    1x1 256-> 64 B=70 12x12              - - res relu         | (1, 64)   | 140 workgroups, % 8 == 4 in the XCD remap      140
    3x3 128-> 64 B=64 12x12              s - -   relu         | (3, 64)   | 128 workgroups, % 8 == 0                       128
    5x5  64->128 B=3  40x40              - t -   -            | (5, 128)  |                                                50
    3x3 448-> 64 B=1   8x8               s t res -            | (3, 64)   | 28 blocks, exactly one tile                      1

  SPLIT_CASES (every case as x6 and as x3)
    3x3  64-> 64 B=3  40x40              s t res relu         | (3, 64, dbh)     | double-buffered halo, 2 block pairs     50
    3x3  48->128 B=5  13x21              s - -   -            | (3, 128, single) | odd block count, single-buffer 3x3 form 18
    3x3  32->128 B=1   5x3               - t res -            | (3, 128, dbh)    | double-buffered halo with ONE pair       1
    3x3  16-> 64 B=2   1x1               - - -   relu         | (3, 64, single)  | single block                             1
    3x3 448-> 64 B=1   8x8               s t -   relu         | (3, 64, dbh)     | 14 pairs                                 1
    3x3 128-> 64 B=64 12x12              - t res relu         | (3, 64, dbh)     | 128 workgroups, % 8 == 0               128
    5x5 128->128 B=2  13x21              s - res -            | (5, 128, single) |                                          6
    5x5  48-> 64 B=3   5x3               - - res relu         | (5, 64, single)  |                                          2
    5x5  16->128 B=1   3x5               s t -   -            | (5, 128, single) |                                          1
    5x5  64-> 64 B=3  40x40              - t -   relu         | (5, 64, single)  |                                         50
    1x1  16-> 64 B=1   1x1               s - res relu         | (1, 64, single)  | S = 1: the ring prologue's `S > 1` is false, no DMA in flight  1
    1x1  32->128 B=5   9x17              - - res -            | (1, 128, single) | S = 2: the third ring slot is never used 18
    1x1 256-> 64 B=70 12x12              s t -   -            | (1, 64, single)  | 140 workgroups, % 8 == 4               140

  BF16_CASES (arith bf16)
    3x3  64-> 64 B=5  40x40              s t res relu         | (3, 64)   | 3 absent slots in the last group               50
    3x3  16->128 B=1   1x1               s - -   -            | (3, 128)  | three empty slots                                1
    5x5  48->128 B=2   5x3               - t res -            | (5, 128)  | 27 tap slots, two of them zero                   1
    5x5 128-> 64 B=6  13x21              - - -   relu         | (5, 64)   | a kernel row per step                           12
    5x5  64->128 B=3  40x40              s t -   -            | (5, 128)  |                                                25
    5x5  16-> 64 B=1   3x5               - t res relu         | (5, 64)   |                                                 1
    3x3 128-> 64 B=74 12x12              s - res -            | (3, 64)   | 76 workgroups, % 8 == 4                         76
    3x3 128->128 B=64 12x12              - - res relu         | (3, 128)  | 64 workgroups, % 8 == 0                         64
    3x3 448-> 64 B=1   8x8               s - -   relu         | (3, 64)   |                                                 1
    1x1  16-> 64 B=1   1x1               - t -   -            | (1, 64)   | S = 1, a 128-item slab: two waves issue          1
    1x1  32->128 B=3  13x21              s t res -            | (1, 128)  | S = 2                                           12
    1x1 256-> 64 B=70 12x12              - - -   relu         | (1, 64)   |                                               140

Yardstick and bar, per image (`check_images`), none of them a new number:
    f32, x6    fp64 on the fp32 operands (`ref_conv`), the project's TOL = 1e-5.
    x3, bf16   an EMULATED reference in fp64 (`ref_emulated`): planes p1 = bf16(v), p2 = bf16(v - p1), round to nearest, as
               `store_halo` and the pack kernel form them; x3 = conv(x1, w1) + conv(x1, w2) + conv(x2, w1), bf16 = conv(x1, w1);
               the epilogue in fp64 on the fp32 scale / shift / res.  The device differs from it only by fp32 accumulation --
               the difference x6 is already held to -- so the bar is the same TOL.  The same launches also keep the bars of
               tests/test_gpu_parity.py test_conv2d_fwd_bf16_split against the TRUE fp64, per image: 1e-4 (x3), 2e-2 (bf16);
               the CPU test asserts that the emulated references alone are inside these.

Measured on an MI355X, worst image over every case of part 1 (`pytest -s` prints the worst and best image of every case):
    f32    against fp64           2.0e-06   (5x5 128 -> 128, B = 2, 13x21)
    x6     against fp64           2.0e-06   (5x5 128 -> 128, B = 2, 13x21)
    x3     against the emulation  1.7e-06   (3x3 448 -> 64, B = 1, 8x8);     true fp64 9.1e-06 (3x3 16 -> 64, B = 2, 1x1)
    bf16   against the emulation  8.5e-07   (5x5 128 -> 64, B = 6, 13x21);   true fp64 3.4e-03 (3x3 16 -> 128, B = 1, 1x1)
  The exact launches of part 2, the pack layouts and the untouched buffers hold with no element off.

2. Exact launches (scale / shift / res NULL, relu 0, compared with == on values).  EXACT_SHAPES: all six (ks, cout) with
cin = 32 plus 3x3 with cin = 48 for both cout -- with the four arithmetics every one of the 28 instances.
  Impulse: image b (B = cin, 9x10 = 2 tiles on each axis) holds one non-zero element v in channel b at IMPULSE_POS[set][b % 16].
  The output is v times the flipped kernel of channel b around that pixel and exactly 0 elsewhere, everything past the border
  included.  Two position sets, each launched with both values of v:
      "edge"   the four corners, both sides of both tile boundaries, pixels on every border.  A tap that reaches outside the
               image is not observed: 3x3 sees 71.5 % of the weight elements, 5x5 60.3 % (`impulse_observed`, asserted).
      "inner"  every pixel at least 2 from the border (y 2..6, x 2..7), several with a window that straddles a tile boundary:
               all ks * ks taps of every channel land inside the image, so EVERY packed weight element (padded tap slots,
               ring slots, both k halves) is observed exactly once, with v = 1 and with the two-plane v.
  `exact_ref` = the fp64 sum of the plane products the arithmetic issues (f32: the fp32 rounding of x * w), which for
      v = 1, general w:                f32 w;  x6 w bit for bit (w1 + w2 + w3 == w);  x3 w1 + w2;  bf16 bf16(w)
      v = 1 + 2^-8 (planes 1, 2^-8, 0), w rounded to 14 significant bits (`round14`):
                                       f32 fl(v * w);  x6 v * w exactly;  x3 w + 2^-8 w1;  bf16 bf16(w)
  Delta weights: w[co, co % cin, co % (ks * ks)] = 1, all else 0, on a general x (DELTA_SHAPES, B = 3, 13x21): output channel co
  is the shifted input channel -- f32 and x6: x bit for bit; x3: x1 + x2; bf16: bf16(x) -- with zeros past the border.
  The CPU test re-derives every expected tensor by an fp32 emulation in the kernel's product order (`PRODUCTS`, compared
  with the PA / PB arrays parsed out of csrc/conv_mfma_split16.hip) and asserts that each of the three low-order products of x6 (x3w1, x1w3, x2w2), dropped, changes an expectation.
3. Pack layouts, bit for bit (`pack_f32_layout`, `pack_bf16s_layout`; PACK_SHAPES).
4. One NaN / Inf element (image 1 of B = 3, 13x21; NF_SHAPES): non-finite inside its ks x ks window in every channel, the bar of
   part 1 everywhere else.
5. Refusals: `mutations` / `pack_mutations`.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from _infer_f16s import PAD, NAN, TOL, cid, ref_conv, check_images, image_max, image_ratio, he, fmt_images      # noqa: F401
from _infer_f16s import ImageMismatch                                                                              # noqa: F401
from _infer_f16s import slice_buffer, nan_output, read_slice                                                       # noqa: F401
from _infer_b16 import FAKE, SIGS, raw                                                                             # noqa: F401
from test_gpu_conv_ex import cb16, nchw, check_outside_untouched                                                   # noqa: F401

ARITHS = ["f32", "x6", "x3", "bf16"]
NSPLIT = {"f32": 0, "x6": 3, "x3": 2, "bf16": 1}
KIND = {"f32": "f32", "x6": "bf16s", "x3": "bf16s", "bf16": "bf16s"}          # the entry point's name in _infer_b16.SIGS
TRUE_BAR = {"f32": TOL, "x6": TOL, "x3": 1e-4, "bf16": 2e-2}                  # against fp64 on the fp32 operands
# the kernel's product order (conv_mfma_split16.hip PA / PB, low-order terms first): (activation plane, weight plane)
PRODUCTS = {"x6": [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], "x3": [(1, 0), (0, 1), (0, 0)], "bf16": [(0, 0)]}

Case = namedtuple("Case", "ks cin cout B H W scale shift res relu offs")
F32_CASES = [
    Case(3, 64, 64, 3, 40, 40, True, True, True, 1, (16, 32, 48)),
    Case(5, 128, 128, 2, 13, 21, True, False, False, 0, (32, 48, 16)),
    Case(1, 16, 64, 1, 1, 1, False, True, True, 0, (48, 16, 32)),
    Case(1, 32, 128, 5, 9, 17, False, False, False, 1, (16, 48, 32)),
    Case(3, 16, 128, 1, 5, 3, True, True, False, 0, (32, 16, 48)),
    Case(5, 48, 64, 2, 1, 1, False, True, True, 1, (48, 32, 16)),
    Case(5, 16, 64, 1, 3, 5, True, False, True, 0, (16, 32, 48)),
    Case(1, 256, 64, 70, 12, 12, False, False, True, 1, (32, 48, 16)),
    Case(3, 128, 64, 64, 12, 12, True, False, False, 1, (48, 16, 32)),
    Case(5, 64, 128, 3, 40, 40, False, True, False, 0, (16, 48, 32)),
    Case(3, 448, 64, 1, 8, 8, True, True, True, 0, (32, 16, 48)),
]
SPLIT_CASES = [
    Case(3, 64, 64, 3, 40, 40, True, True, True, 1, (16, 32, 48)),
    Case(3, 48, 128, 5, 13, 21, True, False, False, 0, (32, 48, 16)),
    Case(3, 32, 128, 1, 5, 3, False, True, True, 0, (48, 16, 32)),
    Case(3, 16, 64, 2, 1, 1, False, False, False, 1, (16, 48, 32)),
    Case(3, 448, 64, 1, 8, 8, True, True, False, 1, (32, 16, 48)),
    Case(3, 128, 64, 64, 12, 12, False, True, True, 1, (48, 32, 16)),
    Case(5, 128, 128, 2, 13, 21, True, False, True, 0, (16, 32, 48)),
    Case(5, 48, 64, 3, 5, 3, False, False, True, 1, (32, 48, 16)),
    Case(5, 16, 128, 1, 3, 5, True, True, False, 0, (48, 16, 32)),
    Case(5, 64, 64, 3, 40, 40, False, True, False, 1, (16, 48, 32)),
    Case(1, 16, 64, 1, 1, 1, True, False, True, 1, (32, 16, 48)),
    Case(1, 32, 128, 5, 9, 17, False, False, True, 0, (48, 32, 16)),
    Case(1, 256, 64, 70, 12, 12, True, True, False, 0, (16, 32, 48)),
]
BF16_CASES = [
    Case(3, 64, 64, 5, 40, 40, True, True, True, 1, (16, 32, 48)),
    Case(3, 16, 128, 1, 1, 1, True, False, False, 0, (32, 48, 16)),
    Case(5, 48, 128, 2, 5, 3, False, True, True, 0, (48, 16, 32)),
    Case(5, 128, 64, 6, 13, 21, False, False, False, 1, (16, 48, 32)),
    Case(5, 64, 128, 3, 40, 40, True, True, False, 0, (32, 16, 48)),
    Case(5, 16, 64, 1, 3, 5, False, True, True, 1, (48, 32, 16)),
    Case(3, 128, 64, 74, 12, 12, True, False, True, 0, (16, 32, 48)),
    Case(3, 128, 128, 64, 12, 12, False, False, True, 1, (32, 48, 16)),
    Case(3, 448, 64, 1, 8, 8, True, False, False, 1, (48, 16, 32)),
    Case(1, 16, 64, 1, 1, 1, False, True, False, 0, (16, 48, 32)),
    Case(1, 32, 128, 3, 13, 21, True, True, True, 0, (32, 16, 48)),
    Case(1, 256, 64, 70, 12, 12, False, False, False, 1, (48, 32, 16)),
]
TABLES = {"f32": F32_CASES, "split": SPLIT_CASES, "bf16": BF16_CASES}
TABLE_ARITHS = {"f32": ["f32"], "split": ["x6", "x3"], "bf16": ["bf16"]}

# part 2
EXACT_SHAPES = [(ks, 32, cout) for ks in (1, 3, 5) for cout in (64, 128)] + [(3, 48, 64), (3, 48, 128)]        # (ks, cin, cout)
IMPULSE_H, IMPULSE_W = 9, 10
IMPULSE_POS = {
    "edge": [(0, 0), (0, 9), (8, 0), (8, 9), (7, 7), (7, 8), (8, 7), (8, 8), (4, 4), (3, 7), (7, 2), (8, 5), (0, 7), (0, 8), (5, 9), (4, 0)],
    "inner": [(2, 2), (6, 7), (2, 7), (6, 2), (4, 7), (6, 4), (5, 6), (3, 3), (6, 6), (4, 2), (2, 5), (5, 7), (3, 6), (6, 3), (4, 4), (2, 4)],
}
IMPULSE_V = {"one": 1.0, "split": 1.0 + 2.0 ** -8}
DELTA_SHAPES = [(3, 32, 128), (5, 32, 128), (1, 64, 64)]
DELTA_B, DELTA_H, DELTA_W = 3, 13, 21
EXACT_OFFS = (32, 16, 48)
# part 3
PACK_SHAPES = [(64, 16, 1), (128, 48, 5), (64, 32, 3), (128, 32, 3)]                                           # (cout, cin, ks)
# part 4: the pixel sits on a tile corner, its window spans four tiles
NF_SHAPES = [(3, 64, 128), (5, 64, 64)]
NF_B, NF_H, NF_W, NF_Y, NF_X, NF_CH = 3, 13, 21, 7, 8, 37


# ---------------------------------------------------------------------------------------------------- launch geometry
def images_per_workgroup(arith, ks):
    """launch_conv (csrc/conv_mfma_f32.hip): 2; launch_bf16s (csrc/conv_mfma_split16.hip, F16 = false): WN = 1, 4 images, for
    one plane and 3x3 / 5x5, else 2."""
    return 4 if arith == "bf16" and ks > 1 else 2


def grid(arith, B, H, W, ks):
    img = images_per_workgroup(arith, ks)
    return -(-B // img) * -(-H // 8) * -(-W // 8)


def case_grid(arith, c):
    return grid(arith, c.B, c.H, c.W, c.ks)


def taps_per_step(ks, cout, ns):
    """csrc/conv_mfma_split16.hip taps_per_step."""
    want = 1 if ns == 3 else (2 if ns == 2 else (3 if cout == 128 else ks))
    return min(want, ks * ks)


def tap_slots(ks, cout, ns):
    """(barrier steps per channel block, taps per step): steps * taps >= ks * ks, the surplus slots hold zero weight."""
    tps = taps_per_step(ks, cout, ns)
    return -(-ks * ks // tps), tps


def slab_items(ks, cout, ns):
    """16-byte items of one step's weight slab ([tap in step][plane][2][cout][8] bf16): a DMA pass moves 256."""
    return taps_per_step(ks, cout, ns) * ns * 2 * cout * 8 * 2 // 16


def steps(arith, ks, cin, cout):
    """S of the kernel: weight slabs (barrier steps) of the whole launch."""
    if arith == "f32":
        return (cin // 16) * ks * ks
    return (cin // 16) * tap_slots(ks, cout, NSPLIT[arith])[0]


def instance(arith, ks, cin, cout):
    """The template instance a shape runs."""
    if arith in ("f32", "bf16"):
        return (arith, ks, cout)
    return (arith, ks, cout, "dbh" if ks == 3 and (cin // 16) % 2 == 0 else "single")


def all_instances():
    out = []
    for a in ARITHS:
        for ks in (1, 3, 5):
            for cout in (64, 128):
                forms = ["dbh", "single"] if a in ("x6", "x3") and ks == 3 else ["single"]
                out += [(a, ks, cout) if a in ("f32", "bf16") else (a, ks, cout, f) for f in forms]
    return out


def case_slices(c):
    """[(slice width, buffer width, offset)] of every slice the case addresses."""
    s = [(c.cin, c.offs[0]), (c.cout, c.offs[1])] + ([(c.cout, c.offs[2])] if c.res else [])
    return [(w, w + PAD, o) for w, o in s]


# ---------------------------------------------------------------------------------------------------- planes, references
def planes(v, n):
    """The n bf16 planes of an fp32 tensor as fp32 values: p_i = bf16(residual), round to nearest; the residual in fp32 (exact)."""
    out, r = [], v.float().clone()
    for _ in range(n):
        q = r.bfloat16().float()
        out.append(q)
        r = r - q
    return out


def conv64(x, w):
    return F.conv2d(x.double(), w.double(), padding=w.shape[2] // 2)


def plane_conv(arith, x, w, products=None):
    """fp64 sum of the plane products the arithmetic issues (f32: the plain convolution of the fp32 operands)."""
    if arith == "f32":
        return conv64(x, w)
    ns = NSPLIT[arith]
    xp, wp = planes(x, ns), planes(w, ns)
    y = None
    for a, b in (PRODUCTS[arith] if products is None else products):
        t = conv64(xp[a], wp[b])
        y = t if y is None else y + t
    return y


def _epilogue(y, scale, shift, res, relu):
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def ref_emulated(arith, x, w, scale=None, shift=None, res=None, relu=0):
    """x3 / bf16: act(sum of the issued plane products * scale + shift + res), everything after the plane split in fp64.
    (x1 is shared: conv(x1, w1) + conv(x1, w2) = conv(x1, w1 + w2), the sum exact in fp64.)"""
    assert arith in ("x3", "bf16")
    ns = NSPLIT[arith]
    xp, wp = planes(x, ns), planes(w, ns)
    if arith == "bf16":
        y = conv64(xp[0], wp[0])
    else:
        y = conv64(torch.cat([xp[0], xp[1]], 1), torch.cat([wp[0].double() + wp[1].double(), wp[0].double()], 1))
    return _epilogue(y, scale, shift, res, relu)


def yardstick(arith, p):
    """(the reference the launch is held to at TOL, fp64 on the fp32 operands)."""
    true = ref_conv(p["x"], p["w"], p["scale"], p["shift"], p["res"], p["relu"])
    if arith in ("f32", "x6"):
        return true, true
    return ref_emulated(arith, p["x"], p["w"], p["scale"], p["shift"], p["res"], p["relu"]), true


def exact_ref(arith, x, w, products=None):
    """Expected values of an exact launch (one non-zero product term per output element), as fp64: f32 = the fp32 rounding of
    the exact product, the split arithmetics = the exact sum of their plane products."""
    y = plane_conv(arith, x, w, products)
    return y.float().double() if arith == "f32" else y


def exact_emulated_f32(arith, x, w):
    """The same expectation by fp32 arithmetic in the kernel's order: acc = 0, then acc += product for every (PA, PB) pair
    (each product term is exact in fp32: 8 x 8 significand bits; f32: one fused multiply-add per term)."""
    if arith == "f32":
        return conv64(x, w).float()
    ns = NSPLIT[arith]
    xp, wp = planes(x, ns), planes(w, ns)
    acc = None
    for a, b in PRODUCTS[arith]:
        t64 = conv64(xp[a], wp[b])
        t = t64.float()
        assert torch.equal(t.double(), t64), "a plane product is exact in fp32"
        acc = t if acc is None else acc + t
    return acc


def round14(w):
    """fp32 values rounded to 14 significant bits (nearest, ties away): two bf16 planes hold them exactly."""
    b = w.contiguous().view(torch.int32)
    return ((b + (1 << 9)) & ~((1 << 10) - 1)).view(torch.float32)


def impulse_input(cin, v, pos):
    """[B = cin][cin][9][10]: image b holds v in channel b at IMPULSE_POS[pos][b % 16]."""
    x = torch.zeros(cin, cin, IMPULSE_H, IMPULSE_W)
    for b in range(cin):
        y, xx = IMPULSE_POS[pos][b % len(IMPULSE_POS[pos])]
        x[b, b, y, xx] = v
    return x


def impulse_operands(ks, cin, cout, vname, pos):
    g = torch.Generator().manual_seed(23000 + ks * 7 + cin + cout)
    w = he(g, cout, cin, ks)
    return impulse_input(cin, IMPULSE_V[vname], pos), (w if vname == "one" else round14(w))


def impulse_observed(ks, cin, cout, pos):
    """Weight elements an impulse launch observes (= its non-zero expectations): cout * the (channel, tap) pairs whose output
    pixel lies inside the image.  "inner": all cout * cin * ks * ks."""
    P, n = ks // 2, 0
    for b in range(cin):
        py, px = IMPULSE_POS[pos][b % len(IMPULSE_POS[pos])]
        n += sum(0 <= py - kh + P < IMPULSE_H and 0 <= px - kw + P < IMPULSE_W for kh in range(ks) for kw in range(ks))
    return cout * n


def delta_weight(ks, cin, cout):
    """w[co, co % cin, co % (ks * ks)] = 1: ci and tap run over all their values as co does."""
    w = torch.zeros(cout, cin, ks * ks)
    co = torch.arange(cout)
    w[co, co % cin, co % (ks * ks)] = 1.0
    return w.view(cout, cin, ks, ks)


def delta_operands(ks, cin, cout):
    g = torch.Generator().manual_seed(24000 + ks * 7 + cin + cout)
    return torch.randn(DELTA_B, cin, DELTA_H, DELTA_W, generator=g) * 3, delta_weight(ks, cin, cout)


# ---------------------------------------------------------------------------------------------------- inputs
def inputs(c, seed=0):
    """CPU operands of one Case (None where the case passes NULL)."""
    g = torch.Generator().manual_seed(21000 + seed + c.ks * 7 + c.cin + c.cout + c.B + c.H)
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g) * 3, w=he(g, c.cout, c.cin, c.ks),
                scale=torch.rand(c.cout, generator=g) + 0.5 if c.scale else None,
                shift=torch.randn(c.cout, generator=g) * 0.3 if c.shift else None,
                res=torch.randn(c.B, c.cout, c.H, c.W, generator=g) if c.res else None, relu=c.relu)


@functools.lru_cache(maxsize=None)
def case_refs(arith, c):
    """(operands, yardstick, true fp64) of a case, computed once and shared (never modified)."""
    p = inputs(c)
    ref, true = yardstick(arith, p)
    return p, ref, true


def nf_case(ks, cin, cout):
    return Case(ks, cin, cout, NF_B, NF_H, NF_W, True, True, True, 0, (32, 48, 16))


# ---------------------------------------------------------------------------------------------------- pack layouts
def pack_f32_layout(w):
    """tsr_pack_conv_weight: [Cin/16][tap][4 (channel quad)][Cout][4] fp32."""
    cout, cin, ks, _ = w.shape
    return w.reshape(cout, cin // 16, 4, 4, ks * ks).permute(1, 4, 2, 0, 3).contiguous().reshape(-1)


def pack_bf16s_layout(w, ns):
    """tsr_pack_conv_weight_bf16s: [Cin/16][step][tap in step][plane][2 (k half)][Cout][8] bf16; plane p = bf16 of the residual
    of the planes before it, padded tap slots exactly zero."""
    cout, cin, ks, _ = w.shape
    nstep, tps = tap_slots(ks, cout, ns)
    T, TP = ks * ks, nstep * tps
    pl = torch.stack(planes(w, ns)).reshape(ns, cout, cin // 16, 2, 8, T)
    pl = F.pad(pl, (0, TP - T))                                             # [plane][co][chunk][kh][j][padded tap]
    return pl.permute(2, 5, 0, 3, 1, 4).contiguous().reshape(-1).bfloat16()


def bf16s_elems(cout, cin, ks, ns):
    """tsr_conv_weight_bf16s_elems: the larger of the padded-tap size and the K = 32 kernel's (channel blocks in pairs)."""
    nstep, tps = tap_slots(ks, cout, ns)
    return max(ns * cout * cin * nstep * tps, ns * cout * ((cin + 31) // 32 * 32) * ks * ks)


def bf16s_written(cout, cin, ks, ns):
    nstep, tps = tap_slots(ks, cout, ns)
    return ns * cout * cin * nstep * tps


# ---------------------------------------------------------------------------------------------------- refusals
REFUSAL_CASE = Case(3, 32, 64, 1, 5, 3, True, True, True, 1, (16, 32, 48))
POINTERS = ["in", "w_packed", "scale", "shift", "res", "out"]


def valid_ints(arith):
    """The integer arguments of the valid argument list (pointers are the caller's)."""
    c = REFUSAL_CASE
    v = {"in_ctot": c.cin + PAD, "in_coff": c.offs[0], "cin": c.cin, "cout": c.cout, "ks": c.ks, "res_ctot": c.cout + PAD,
         "res_coff": c.offs[2], "out_ctot": c.cout + PAD, "out_coff": c.offs[1], "relu": c.relu, "B": c.B, "H": c.H, "W": c.W}
    if arith != "f32":
        v["nsplit"] = NSPLIT[arith]
    return v


def mutations(arith):
    """[(name, overrides of the valid list)]: every argument list the entry point must refuse with status 1."""
    c = REFUSAL_CASE
    cin, cout = c.cin, c.cout
    m = [(f"NULL {p}", {p: None}) for p in ("in", "w_packed", "out")]
    m += [(f"{d} = {v}", {d: v}) for d in ("B", "H", "W") for v in (0, -1)]
    m += [("cin = 0", {"cin": 0}), ("cin negative", {"cin": -16}), ("cin + 8", {"cin": cin + 8}),
          ("in_ctot - 8", {"in_ctot": cin + PAD - 8}), ("in_coff 8", {"in_coff": 8}), ("out_ctot - 8", {"out_ctot": cout + PAD - 8}),
          ("out_coff 24", {"out_coff": 24}), ("res_ctot - 8", {"res_ctot": cout + PAD - 8}), ("res_coff 8", {"res_coff": 8}),
          ("in_coff negative", {"in_coff": -16}), ("out_coff negative", {"out_coff": -16}), ("res_coff negative", {"res_coff": -16}),
          ("in_coff -cin", {"in_coff": -cin}), ("res_coff -cout", {"res_coff": -cout}),
          ("in slice past the end", {"in_coff": PAD + 16}), ("out slice past the end", {"out_coff": PAD + 16}),
          ("res slice past the end", {"res_coff": PAD + 16}),
          ("in buffer narrower than cin", {"in_ctot": cin - 16, "in_coff": 0}),
          ("out buffer narrower than cout", {"out_ctot": cout - 16, "out_coff": 0}),
          ("res buffer narrower than cout", {"res_ctot": cout - 16, "res_coff": 0})]
    m += [(f"cout = {v}", {"cout": v}) for v in (0, 16, 32, 96, 256, -64)]
    m += [(f"ks = {v}", {"ks": v}) for v in (-3, 0, 2, 4, 7)]
    if arith != "f32":
        m += [(f"nsplit = {v}", {"nsplit": v}) for v in (0, 4, -1, -2)]
    return m


def pack_mutations(kind):
    """(valid integer arguments, [(name, overrides)]) of "pack_f32" / "pack_bf16s" (pointers `w`, `w_packed` are the caller's)."""
    base = {"cout": 64, "cin": 32, "ks": 3}
    m = [("NULL w", {"w": None}), ("NULL w_packed", {"w_packed": None})]
    m += [(f"cout = {v}", {"cout": v}) for v in (0, 32, 96, 256, -64)] + [(f"ks = {v}", {"ks": v}) for v in (-3, 0, 2, 4, 7)]
    m += [("cin = 0", {"cin": 0}), ("cin negative", {"cin": -16}), ("cin + 8", {"cin": 40})]
    if kind == "pack_bf16s":
        base["nsplit"] = 3
        m += [(f"nsplit = {v}", {"nsplit": v}) for v in (0, 4, -1, -2)]
    return base, m


# ---------------------------------------------------------------------------------------------------- packs (GPU)
def _L():
    from tactilesr_amd import _lib
    return _lib


def pack_f32(w):
    L = _L()
    cout, cin, ks, _ = w.shape
    wd = w.cuda().contiguous()
    wp = torch.zeros(w.numel(), device="cuda")
    L.call("tsr_pack_conv_weight", L.ptr(wd), L.ptr(wp), L.c_int(cout), L.c_int(cin), L.c_int(ks), L.stream())
    torch.cuda.synchronize()
    return wp


def pack_bf16s(w, ns):
    L = _L()
    cout, cin, ks, _ = w.shape
    wd = w.cuda().contiguous()
    wp = torch.zeros(L.load().tsr_conv_weight_bf16s_elems(cout, cin, ks, ns), dtype=torch.bfloat16, device="cuda")
    L.call("tsr_pack_conv_weight_bf16s", L.ptr(wd), L.ptr(wp), L.c_int(cout), L.c_int(cin), L.c_int(ks), L.c_int(ns), L.stream())
    torch.cuda.synchronize()
    return wp


def pack(arith, w):
    return pack_f32(w) if arith == "f32" else pack_bf16s(w, NSPLIT[arith])
