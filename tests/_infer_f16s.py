"""Case tables, layouts, fp64 references and the per-image checker of tests/test_gpu_infer_fp16x3.py -- everything that runs
without a GPU (tests/test_infer_f16s_cpu.py checks the references, the checker and the tables), plus the pack calls of the
fp16x3 inference launches (`tactilesr_amd._lib` is imported inside them, never at module level), and the REFUSAL TABLES of the
three launches and of the pack routines (the end of this file): the GPU test sends them to real buffers and checks that a
refused call wrote nothing, the CPU test sends them with fake pointers and checks the status alone.

The launches under test are the INFERENCE instantiations (`EXT = false`) behind `conv_impl = "fp16x3"`:

    tsr_conv2d_fwd_f16s          3x3 / 5x5: conv_mfma_k32.hip, 256 threads; C_out 64 = 4 images per workgroup, C_out 128 = 2
                                 (the 512-thread, 4-image form of C_out 128 is the TRAIN instantiation's);
                                 1x1: conv_mfma_split16.hip, 2 images per workgroup
    tsr_conv2d_fwd_f16s_pair     conv_mfma_k32.hip PAIR form, 2 images per workgroup
    tsr_conv2d_fwd_f16s_fuse1x1  conv_mfma_k32.hip FUSE2 form for every C_in (`use_k32` sends nothing elsewhere), 2 images

Every kernel remaps blockIdx over 8 XCDs (`q = nwg >> 3, r = nwg & 7`); `grid()` below is the launchers' own arithmetic,
ceil(B / images) * ceil(H / 8) * ceil(W / 8).

Every case: input, output and residual slices at three different non-zero channel offsets (16 / 32 / 48, in that order in
`offs`) in buffers 48 channels wider than the slice (offset 48 = the slice ends the buffer), NaN everywhere else.  Epilogue
settings and the out_amax setting rotate over the cases.  out_amax settings: None = NULL pointer, "zero" = prior 0 (the slot
must end as max|got| exactly), "big" = prior 1e6 (must survive bit for bit), "half" = prior 0.5 max|ref| (must be raised to
max|got|).

  F16S_CASES (tsr_conv2d_fwd_f16s)     epilogue / out_amax          | why                                          grid
    3x3  64-> 64 B=3  40x40            scale+shift, res, relu, zero | network shape, one absent slot of 4             25
    5x5 128->128 B=2  13x21            scale, no res, no relu, big  | ragged on both axes                              6
    1x1 256-> 64 B=5   9x17            shift, res, relu, NULL       | split16 1x1 form, 2 images, last group half empty 18
    3x3  16->128 B=1   5x3             neither, no res, relu, half  | ONE channel block, zero-padded block pair, < one tile 1
    5x5  48-> 64 B=2   1x1             both, res, no relu, half     | odd block count, image smaller than the halo     1
    1x1 128->128 B=3  13x21            scale, res, no relu, zero    | 1x1 with 128 output channels                    12
    3x3 128-> 64 B=70 12x12            shift, no res, relu, big     | 18 groups x 4 tiles = 72 workgroups = 9 * 8     72
    3x3 128-> 64 B=74 12x12            neither, res, no relu, zero  | 19 groups x 4 tiles = 76: k32 grid % 8 == 4     76
    1x1  64-> 64 B=70 12x12            neither, res, relu, half     | 35 x 4 = 140 workgroups, % 8 == 4              140
    5x5  64->128 B=3  40x40            both, no res, relu, NULL     | 5x5 x 128 channels (inference: 2 images, 256 threads) 50
    3x3 448-> 64 B=1   8x8             scale, res, relu, zero       | T = 7 fuse width (28 blocks), exactly one tile   1
    1x1  64->128 B=1   1x1             shift, no res, no relu, big  | 1x1 image on the 1x1 form                        1

  PAIR_CASES (tsr_conv2d_fwd_f16s_pair; expected tensor in tsr_pair_channel_perm order)
    C_in  64 B=3  40x40  scale+shift, relu, zero    | network shape, second slot of the last group absent        50
    C_in  16 B=1   1x1   scale, no relu, big        | one channel block (padded pair), image smaller than the halo 1
    C_in  32 B=5   5x3   shift, relu, half          | one block pair, less than one tile                          3
    C_in  48 B=3   9x17  neither, no relu, NULL     | odd block count                                            12
    C_in 128 B=5  13x21  scale+shift, no relu, half | four block pairs, ragged on both axes                      18
    C_in  64 B=1  13x21  neither, relu, zero        | B = 1: second image slot of every workgroup absent          6
    C_in  32 B=37  9x17  scale, relu, NULL          | 19 groups x 6 tiles = 114 workgroups, % 8 == 2            114
    C_in 128 B=3   5x3   shift, relu, big           |                                                             2
    C_in  48 B=1  40x40  scale+shift, relu, zero    | odd block count at the network's image size                25

  FUSE_CASES (tsr_conv2d_fwd_f16s_fuse1x1; (shift2, res, relu2) takes all eight combinations)
    3x3 128 B=2 40x40  relu, scale+shift, (1,1,0) zero | the model's first launch (w2 = W_a, shift2 = b_c, res = x)    25
    5x5 128 B=5 40x40  relu, scale+shift, (0,1,1) half | the model's second launch (res = P, relu2); 3 groups x 25     75
    3x3  16 B=1  1x1   no relu, scale,    (0,0,0) big  | one channel block, 1x1 image                                  1
    5x5  48 B=2  5x3   relu, shift,       (1,0,1) NULL | odd block count, less than one tile                           1
    3x3  48 B=5 13x21  no relu, neither,  (1,1,1) zero | odd block count, ragged, last group half empty               18
    5x5  16 B=1 13x21  relu, scale+shift, (0,0,1) half | one channel block, B = 1                                      6
    3x3 128 B=5  5x3   relu, scale+shift, (1,0,0) big  |                                                               3
    5x5 128 B=2  1x1   no relu, scale+shift, (0,1,0) zero | image smaller than the halo                                1

Bar: the project's TOL = 1e-5 against fp64 on the fp32 operands, PER IMAGE (`check_images`): max|got_b - ref_b| / max|ref_b|.
Inputs are randn * 3 per image without outlier, and every case asserts max_b max|ref_b| / min_b max|ref_b| < 4 on the CPU,
so the per-image bar is the tensor-wide bar of tests/test_gpu_parity.py up to that factor and not a tighter one.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from test_gpu_conv_ex import cb16, nchw, check_outside_untouched          # noqa: F401  (re-exported)

TOL = 1e-5
PAD = 48                                # every buffer is this many channels wider than its slice
NAN = float("nan")
AMAX_BIG = 1.0e6

F16sCase = namedtuple("F16sCase", "ks cin cout B H W scale shift res relu amax offs")
F16S_CASES = [
    F16sCase(3, 64, 64, 3, 40, 40, True, True, True, 1, "zero", (16, 32, 48)),
    F16sCase(5, 128, 128, 2, 13, 21, True, False, False, 0, "big", (32, 48, 16)),
    F16sCase(1, 256, 64, 5, 9, 17, False, True, True, 1, None, (48, 16, 32)),
    F16sCase(3, 16, 128, 1, 5, 3, False, False, False, 1, "half", (16, 48, 32)),
    F16sCase(5, 48, 64, 2, 1, 1, True, True, True, 0, "half", (32, 16, 48)),
    F16sCase(1, 128, 128, 3, 13, 21, True, False, True, 0, "zero", (48, 32, 16)),
    F16sCase(3, 128, 64, 70, 12, 12, False, True, False, 1, "big", (16, 32, 48)),
    F16sCase(3, 128, 64, 74, 12, 12, False, False, True, 0, "zero", (32, 48, 16)),
    F16sCase(1, 64, 64, 70, 12, 12, False, False, True, 1, "half", (48, 16, 32)),
    F16sCase(5, 64, 128, 3, 40, 40, True, True, False, 1, None, (16, 48, 32)),
    F16sCase(3, 448, 64, 1, 8, 8, True, False, True, 1, "zero", (32, 16, 48)),
    F16sCase(1, 64, 128, 1, 1, 1, False, True, False, 0, "big", (48, 32, 16)),
]

PairCase = namedtuple("PairCase", "cin B H W scale shift relu amax offs")
PAIR_CASES = [
    PairCase(64, 3, 40, 40, True, True, 1, "zero", (16, 32)),
    PairCase(16, 1, 1, 1, True, False, 0, "big", (32, 48)),
    PairCase(32, 5, 5, 3, False, True, 1, "half", (48, 16)),
    PairCase(48, 3, 9, 17, False, False, 0, None, (16, 48)),
    PairCase(128, 5, 13, 21, True, True, 0, "half", (32, 16)),
    PairCase(64, 1, 13, 21, False, False, 1, "zero", (48, 32)),
    PairCase(32, 37, 9, 17, True, False, 1, None, (16, 32)),
    PairCase(128, 3, 5, 3, False, True, 1, "big", (32, 48)),
    PairCase(48, 1, 40, 40, True, True, 1, "zero", (48, 16)),
]

FuseCase = namedtuple("FuseCase", "ks cin B H W relu scale shift shift2 res relu2 amax offs")
FUSE_CASES = [
    FuseCase(3, 128, 2, 40, 40, 1, True, True, True, True, 0, "zero", (16, 32, 48)),
    FuseCase(5, 128, 5, 40, 40, 1, True, True, False, True, 1, "half", (32, 48, 16)),
    FuseCase(3, 16, 1, 1, 1, 0, True, False, False, False, 0, "big", (48, 16, 32)),
    FuseCase(5, 48, 2, 5, 3, 1, False, True, True, False, 1, None, (16, 48, 32)),
    FuseCase(3, 48, 5, 13, 21, 0, False, False, True, True, 1, "zero", (32, 16, 48)),
    FuseCase(5, 16, 1, 13, 21, 1, True, True, False, False, 1, "half", (48, 32, 16)),
    FuseCase(3, 128, 5, 5, 3, 1, True, True, True, False, 0, "big", (16, 32, 48)),
    FuseCase(5, 128, 2, 1, 1, 0, True, True, False, True, 0, "zero", (32, 48, 16)),
]

# the scale contract runs on one launch of every kind at 13x21, B = 3
CONTRACT_KINDS = ["k32_3x3", "1x1", "pair", "fuse1x1"]
CONTRACT_B, CONTRACT_H, CONTRACT_W = 3, 13, 21
HOMOGENEITY_K = [-60, -20, 20, 60]


def cid(c):
    """pytest id of a case: its fields joined by '-' (None -> x, a bool -> 0 / 1, the offsets run together)."""
    def one(v):
        if isinstance(v, tuple):
            return "".join(map(str, v))
        return "x" if v is None else str(int(v) if isinstance(v, bool) else v)
    return "-".join(one(v) for v in c)


# ---------------------------------------------------------------------------------------------------- launch geometry
def images_per_workgroup(kind, ks=3, cout=64):
    """The inference launchers' images per workgroup (csrc/conv_mfma_k32.hip launch_k32 with EXT = false: `IMG = 4 / WN`,
    WN = C_out / 64; csrc/conv_mfma_split16.hip launch_bf16s 1x1: 2; pair and fuse1x1: `(B + 1) / 2`)."""
    if kind == "f16s" and ks > 1 and cout == 64:
        return 4
    return 2


def grid(kind, B, H, W, ks=3, cout=64):
    img = images_per_workgroup(kind, ks, cout)
    return -(-B // img) * -(-H // 8) * -(-W // 8)


def case_grid(c):
    if isinstance(c, F16sCase):
        return grid("f16s", c.B, c.H, c.W, c.ks, c.cout)
    return grid("pair" if isinstance(c, PairCase) else "fuse1x1", c.B, c.H, c.W)


def case_slices(c):
    """[(slice width, buffer width, offset)] of every slice the case addresses."""
    if isinstance(c, F16sCase):
        s = [(c.cin, c.offs[0]), (c.cout, c.offs[1])] + ([(c.cout, c.offs[2])] if c.res else [])
    elif isinstance(c, PairCase):
        s = [(c.cin, c.offs[0]), (128, c.offs[1])]
    else:
        s = [(c.cin, c.offs[0]), (64, c.offs[1])] + ([(64, c.offs[2])] if c.res else [])
    return [(w, w + PAD, o) for w, o in s]


# ---------------------------------------------------------------------------------------------------- layouts
def slice_buffer(x, coff):
    """NCHW (cpu) -> NaN-filled CB16 device buffer of C + PAD channels with x at channel offset coff."""
    return cb16(x, x.shape[1] + PAD, coff)


def nan_output(B, c, H, W):
    return torch.full((B * (c + PAD) * H * W,), NAN, device="cuda")


def read_slice(buf, B, c, H, W, coff):
    """(the slice as NCHW, the whole buffer as NCHW) of a CB16 device buffer of c + PAD channels; asserts that everything
    outside the slice is still NaN."""
    full = nchw(buf, B, c + PAD, H, W)
    check_outside_untouched(full, coff, c)
    return full[:, coff:coff + c].contiguous(), full


# ---------------------------------------------------------------------------------------------------- fp64 references
def _cv(v):
    return v.double().view(1, -1, 1, 1)


def ref_conv(x, w, scale=None, shift=None, res=None, relu=0):
    """act(conv2d(x, w, stride 1, pad k/2) * scale + shift + res) in fp64 on the fp32 operands."""
    y = F.conv2d(x.double(), w.double(), padding=w.shape[2] // 2)
    if scale is not None:
        y = y * _cv(scale)
    if shift is not None:
        y = y + _cv(shift)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def pair_perm():
    """include/tactilesr_hip.h, tsr_pair_channel_perm: kernel channel k = wn * 64 + nt * 16 + c holds channel
    (nt < 2 ? 0 : 64) + wn * 32 + (nt & 1) * 16 + c of torch.cat([conv3, conv5], 1).  (The GPU test compares the library's.)"""
    return torch.tensor([(0 if ((k >> 4) & 3) < 2 else 64) + (k >> 6) * 32 + ((k >> 4) & 1) * 16 + (k & 15) for k in range(128)])


def ref_pair(x, w3, w5, scale=None, shift=None, relu=0, perm=None):
    """The stage-1 pair in the KERNEL's channel order: cat([conv3x3, conv5x5], 1)[:, perm] with scale / shift (given in the
    kernel's order, as the launch takes them) and ReLU."""
    perm = pair_perm() if perm is None else perm
    y = torch.cat([F.conv2d(x.double(), w3.double(), padding=1), F.conv2d(x.double(), w5.double(), padding=2)], 1)[:, perm]
    if scale is not None:
        y = y * _cv(scale)
    if shift is not None:
        y = y + _cv(shift)
    return F.relu(y) if relu else y


def ref_fuse1x1(x, w, scale, shift, relu, w2, shift2=None, res=None, relu2=0):
    """act2(w2 . act(conv(x, w) * scale + shift) + shift2 + res): the stage-2 conv (-> 128) with its fused 64x128 1x1."""
    a = ref_conv(x, w, scale, shift, None, relu)
    return ref_conv(a, w2.double().view(64, 128, 1, 1), None, shift2, res, relu2)


# ---------------------------------------------------------------------------------------------------- per-image checker
class ImageMismatch(AssertionError):
    def __init__(self, image, tile, block, err, tol, what):
        self.image, self.tile, self.block, self.err = image, tile, block, err
        super().__init__(f"{what}: image {image}, 8x8 tile (y {tile[0]}, x {tile[1]}), 16-channel block {block}: "
                         f"{err:.3e} of the image's max|ref| (bar {tol:.1e})")


def image_max(ref):
    return ref.double().abs().amax(dim=(1, 2, 3))


def image_ratio(ref):
    m = image_max(ref)
    return float(m.max() / m.min())


def check_images(got, ref, tol=TOL):
    """max|got_b - ref_b| / max|ref_b| < tol for every image b; returns the per-image errors.  On failure (or a non-finite
    output) raises ImageMismatch naming the worst (image, 8x8 tile, 16-channel block).  For tensors whose images are drawn
    from one distribution (see `image_ratio`)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    B = ref.shape[0]
    e = (got.double() - ref.double()).abs() / image_max(ref).clamp_min(1e-30).view(B, 1, 1, 1)
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    per = e.amax(dim=(1, 2, 3))
    if not bool((per < tol).all()):
        b, c, y, x = (int(v) for v in torch.unravel_index(e.argmax(), e.shape))
        raise ImageMismatch(b, (y // 8, x // 8), c // 16, float(e[b, c, y, x]), tol,
                            "non-finite output" if math.isinf(float(e[b, c, y, x])) else "error above the bar")
    return per


def fmt_images(per):
    return f"worst image {float(per.max()):.1e}, best {float(per.min()):.1e}"


# ---------------------------------------------------------------------------------------------------- inputs
def he(g, cout, cin, ks):
    return torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5


def f16s_inputs(c, seed=0):
    """CPU operands of one F16sCase (None where the case passes NULL)."""
    g = torch.Generator().manual_seed(5000 + seed + c.ks * 7 + c.cin + c.cout + c.B + c.H)
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g) * 3, w=he(g, c.cout, c.cin, c.ks),
                scale=torch.rand(c.cout, generator=g) + 0.5 if c.scale else None,
                shift=torch.randn(c.cout, generator=g) * 0.3 if c.shift else None,
                res=torch.randn(c.B, c.cout, c.H, c.W, generator=g) if c.res else None, relu=c.relu)


def f16s_ref(p):
    return ref_conv(p["x"], p["w"], p["scale"], p["shift"], p["res"], p["relu"])


def pair_inputs(c, seed=0):
    g = torch.Generator().manual_seed(6000 + seed + c.cin + 7 * c.B + c.H)
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g) * 3, w3=he(g, 64, c.cin, 3), w5=he(g, 64, c.cin, 5),
                scale=torch.rand(128, generator=g) + 0.5 if c.scale else None,
                shift=torch.randn(128, generator=g) * 0.3 if c.shift else None, relu=c.relu)


def pair_ref(p):
    return ref_pair(p["x"], p["w3"], p["w5"], p["scale"], p["shift"], p["relu"])


def fuse_inputs(c, seed=0):
    g = torch.Generator().manual_seed(7000 + seed + c.ks * 31 + c.cin + c.B + c.H)
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g) * 3, w=he(g, 128, c.cin, c.ks),
                scale=torch.rand(128, generator=g) + 0.5 if c.scale else None,
                shift=torch.randn(128, generator=g) * 0.3 if c.shift else None, relu=c.relu,
                w2=torch.randn(64, 128, 1, 1, generator=g) * (2.0 / 128) ** 0.5,
                shift2=torch.randn(64, generator=g) * 0.2 if c.shift2 else None,
                res=torch.randn(c.B, 64, c.H, c.W, generator=g) if c.res else None, relu2=c.relu2)


def fuse_ref(p):
    return ref_fuse1x1(p["x"], p["w"], p["scale"], p["shift"], p["relu"], p["w2"], p["shift2"], p["res"], p["relu2"])


def amax_prior(setting, ref):
    """The value the out_amax slot is preset to (None: the launch gets a NULL pointer)."""
    return {None: None, "zero": 0.0, "big": AMAX_BIG, "half": 0.5 * float(ref.abs().max())}[setting]


def check_amax(setting, prior, am, got):
    """The slot is only ever raised: prior 0 -> max|got| exactly; 1e6 survives bit for bit; half the maximum is raised."""
    if setting is None:
        return
    mx = float(got.abs().max())
    if setting == "big":
        assert mx < AMAX_BIG and am.item() == AMAX_BIG, (am.item(), mx)
    else:
        assert prior < mx and am.item() == mx, (prior, am.item(), mx)


# ---------------------------------------------------------------------------------------------------- weight scale, packs
def host_wscale(*ws):
    """2^(13 - floor(log2 max|w|)): max|w| * wscale in [2^13, 2^14) (1 for an all-zero weight, as the device-side pack)."""
    mx = max(float(w.abs().max()) for w in ws)
    return 2.0 ** (13 - math.floor(math.log2(mx))) if mx > 0 else 1.0


def _ctx():
    from tactilesr_amd import _lib
    return _lib


def pack_f16s(w, wscale=None):
    """tsr_pack_conv_weight_f16s with the host-side scale -> (packed fp16 buffer, w_inv_scale)."""
    L = _ctx()
    cout, cin, ks, _ = w.shape
    ws = host_wscale(w) if wscale is None else wscale
    wd = w.cuda().contiguous()
    wp = torch.zeros(L.load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 2), dtype=torch.float16, device="cuda")
    L.call("tsr_pack_conv_weight_f16s", L.ptr(wd), L.ptr(wp), L.c_int(cout), L.c_int(cin), L.c_int(ks), L.c_float(ws), L.stream())
    torch.cuda.synchronize()
    return wp, 1.0 / ws


def pack_f16s_dev(w):
    """tsr_pack_conv_weight_f16s_dev: the scale derived on the device from w_amax[0] = max|w|."""
    L = _ctx()
    cout, cin, ks, _ = w.shape
    wd = w.cuda().contiguous()
    wa = wd.abs().max().reshape(1)
    wp = torch.zeros(L.load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 2), dtype=torch.float16, device="cuda")
    L.call("tsr_pack_conv_weight_f16s_dev", L.ptr(wd), L.ptr(wp), L.c_int(cout), L.c_int(cin), L.c_int(ks), L.ptr(wa), L.stream())
    torch.cuda.synchronize()
    return wp


def pack_pair(w3, w5, dev=False):
    """tsr_pack_conv_weight_pair_f16s with wscale (dev = False) or with a device w_amax = max(max|w3|, max|w5|) -> (packed, w_inv_scale)."""
    L = _ctx()
    cin = w3.shape[1]
    ws = host_wscale(w3, w5)
    w3d, w5d = w3.cuda().contiguous(), w5.cuda().contiguous()
    wa = torch.maximum(w3d.abs().max(), w5d.abs().max()).reshape(1) if dev else None
    wp = torch.zeros(L.load().tsr_conv_weight_pair_elems(cin), dtype=torch.float16, device="cuda")
    L.call("tsr_pack_conv_weight_pair_f16s", L.ptr(w3d), L.ptr(w5d), L.ptr(wp), L.c_int(cin), L.c_float(0.0 if dev else ws),
           L.ptr(wa), L.stream())
    torch.cuda.synchronize()
    return wp, 1.0 / ws


def pack_w2(w2):
    """The 64x128 1x1 half of `confusion` for tsr_conv2d_fwd_f16s_fuse1x1: tsr_pack_conv_weight_f16s of [64][128][1][1]."""
    return pack_f16s(w2.reshape(64, 128, 1, 1))


# ---------------------------------------------------------------------------------------------------- refusals
# Argument lists (name:type, p = pointer, i = int, f = float; the stream comes last) of the entry points under test.
F16S_SIG = ["in:p", "in_ctot:i", "in_coff:i", "cin:i", "w_packed:p", "cout:i", "ks:i", "w_inv_scale:f", "in_amax:p", "out_amax:p",
            "scale:p", "shift:p", "res:p", "res_ctot:i", "res_coff:i", "out:p", "out_ctot:i", "out_coff:i", "relu:i", "B:i", "H:i", "W:i"]
PAIR_SIG = ["in:p", "in_ctot:i", "in_coff:i", "cin:i", "w_packed:p", "w_inv_scale:f", "in_amax:p", "out_amax:p", "scale:p", "shift:p",
            "out:p", "out_ctot:i", "out_coff:i", "relu:i", "B:i", "H:i", "W:i"]
FUSE_SIG = ["in:p", "in_ctot:i", "in_coff:i", "cin:i", "w_packed:p", "ks:i", "w_inv_scale:f", "in_amax:p", "out_amax:p", "scale:p",
            "shift:p", "relu:i", "w2_packed:p", "w2_inv_scale:f", "shift2:p", "res:p", "res_ctot:i", "res_coff:i", "out:p",
            "out_ctot:i", "out_coff:i", "relu2:i", "B:i", "H:i", "W:i"]
PACK_SIG = ["w:p", "w_packed:p", "cout:i", "cin:i", "ks:i", "wscale:f"]
PACK_DEV_SIG = ["w:p", "w_packed:p", "cout:i", "cin:i", "ks:i", "w_amax:p"]
PACK_PAIR_SIG = ["w3:p", "w5:p", "w_packed:p", "cin:i", "wscale:f", "w_amax:p"]
_DGRAD = ["w:p", "w_packed:p", "cout:i", "cin:i", "ks:i", "ci0:i", "nprime:i"]
DGRAD_PACK_SIGS = {
    "tsr_pack_conv_weight_dgrad": _DGRAD,
    "tsr_pack_conv_weight_dgrad_bf16s": _DGRAD + ["nsplit:i"],
    "tsr_pack_conv_weight_dgrad_f16s": _DGRAD + ["wscale:f"],
    "tsr_pack_conv_weight_dgrad_f16s_dev": _DGRAD + ["w_amax:p"],
    "tsr_pack_conv_weight_dgrad_b16k": _DGRAD,
}
LAUNCHES = {"f16s": ("tsr_conv2d_fwd_f16s", F16S_SIG), "pair": ("tsr_conv2d_fwd_f16s_pair", PAIR_SIG),
            "fuse1x1": ("tsr_conv2d_fwd_f16s_fuse1x1", FUSE_SIG)}
FAKE = 16                               # a non-NULL pointer value that is never dereferenced (the CPU test's)
BAD_SCALES = [0.0, -1.0, NAN]

# The valid argument list every launch's refusal test starts from: B = 1, a 5x3 image, one channel block in.
REFUSAL_CASES = {"f16s": F16sCase(3, 16, 64, 1, 5, 3, True, True, True, 1, "zero", (16, 32, 48)),
                 "pair": PairCase(16, 1, 5, 3, True, True, 1, "zero", (16, 32)),
                 "fuse1x1": FuseCase(3, 16, 1, 5, 3, 1, True, True, True, True, 1, "zero", (16, 32, 48))}
REFUSAL_WIDTH = {"f16s": 64, "pair": 128, "fuse1x1": 64}          # channels of `out` (and `res`)


def slice_mutations(cin, cout, with_res=True):
    """Overrides that make a slice description invalid: not a multiple of 16, or leaving its buffer on either side."""
    m = [{"cin": cin + 8}, {"cin": 0}, {"cin": -16}, {"in_ctot": cin + PAD - 8}, {"in_coff": 8}, {"out_ctot": cout + PAD - 8},
         {"out_coff": 24}, {"in_coff": PAD + 16}, {"in_coff": -16}, {"out_coff": PAD + 16}, {"out_coff": -16},
         {"in_ctot": cin - 16, "in_coff": 0}, {"out_ctot": cout - 16, "out_coff": 0}]
    if with_res:
        m += [{"res_ctot": cout + PAD - 8}, {"res_coff": 8}, {"res_coff": PAD + 16}, {"res_coff": -16},
              {"res_ctot": cout - 16, "res_coff": 0}]
    return m


def common_mutations(required):
    return ([{k: None} for k in required] + [{d: v} for d in ("B", "H", "W") for v in (0, -1)]
            + [{"w_inv_scale": v} for v in BAD_SCALES])


def launch_mutations(kind):
    """Every argument list the launch of `kind` must refuse with status 1, as overrides of its valid list."""
    if kind == "f16s":
        return (common_mutations(["in", "w_packed", "out", "in_amax"]) + slice_mutations(16, 64)
                + [{"cout": v} for v in (0, 32, 96, 256)] + [{"ks": v} for v in (-3, 0, 2, 4, 7)])
    if kind == "pair":
        return common_mutations(["in", "w_packed", "out", "in_amax"]) + slice_mutations(16, 128, with_res=False)
    return (common_mutations(["in", "w_packed", "out", "in_amax", "w2_packed"]) + slice_mutations(16, 64)
            + [{"w2_inv_scale": v} for v in BAD_SCALES] + [{"ks": v} for v in (-3, 0, 1, 2, 4, 7)])


def fake_launch_args(kind):
    """The valid list of `kind` with fake pointers everywhere (the integers are those of the GPU test's list)."""
    c = REFUSAL_CASES[kind]
    width = REFUSAL_WIDTH[kind]
    v = {"in_ctot": c.cin + PAD, "in_coff": c.offs[0], "cin": c.cin, "out_ctot": width + PAD, "out_coff": c.offs[1], "relu": c.relu,
         "B": c.B, "H": c.H, "W": c.W, "w_inv_scale": 2.0 ** -14, "w2_inv_scale": 2.0 ** -14, "relu2": 1}
    if kind != "pair":
        v.update(res_ctot=width + PAD, res_coff=c.offs[2], ks=c.ks)
    if kind == "f16s":
        v.update(cout=c.cout)
    v.update({s.split(":")[0]: FAKE for s in LAUNCHES[kind][1] if s.endswith(":p")})
    return v


# the pack routines: (cout, cin, ks) of the valid lists (the last is fuse1x1's 1x1 half), the pair pack's cin
PACK_SHAPES = [(64, 16, 3), (128, 32, 5), (64, 128, 1)]
PACK_PAIR_CIN = 32


def pack_shape_mutations(cin):
    return [{"cin": cin + 8}, {"cin": 0}, {"cin": -16}, {"cout": 0}, {"cout": 32}, {"cout": 96}, {"cout": 256},
            {"ks": -3}, {"ks": 0}, {"ks": 2}, {"ks": 4}, {"ks": 7}, {"w": None}, {"w_packed": None}]


def pack_host_mutations(cin):
    """tsr_pack_conv_weight_f16s"""
    return pack_shape_mutations(cin) + [{"wscale": v} for v in BAD_SCALES]


def pack_dev_mutations(cin):
    """tsr_pack_conv_weight_f16s_dev"""
    return pack_shape_mutations(cin) + [{"w_amax": None}]


def pack_pair_mutations(cin):
    """tsr_pack_conv_weight_pair_f16s (valid list: wscale > 0, w_amax NULL)"""
    return ([{"w3": None}, {"w5": None}, {"w_packed": None}, {"cin": cin + 8}, {"cin": 0}, {"cin": -16}]
            + [{"wscale": v} for v in BAD_SCALES])


# dgrad packs: the gradient of input channels [ci0, ci0 + nprime) of a conv with OIHW weight [cout][cin][ks][ks]
DGRAD_PACK_VALID = {"cout": 64, "cin": 192, "ks": 3, "ci0": 64, "nprime": 128, "nsplit": 3, "wscale": 2.0 ** 14}


def dgrad_pack_mutations(name):
    m = [{"w": None}, {"w_packed": None}, {"cout": 72}, {"cout": 8}, {"nprime": 0}, {"nprime": 32}, {"nprime": 96}, {"nprime": 256},
         {"ci0": -16}, {"ci0": -128}, {"ci0": 80}, {"ci0": 192}, {"cin": 128}, {"ks": -3}, {"ks": 0}, {"ks": 2}, {"ks": 4}, {"ks": 7}]
    if name.endswith("_dev"):
        m.append({"w_amax": None})
    return m


def raw_fake(name, sig, vals):
    """Status of entry point `name` for `vals` (name -> None / fake pointer value / int / float), NULL stream: never reaches
    a device unless every check passes (then, without a device, the launch fails with status 2)."""
    import ctypes
    from tactilesr_amd import _lib
    args = []
    for s in sig:
        n, t = s.split(":")
        v = vals[n]
        args.append(ctypes.c_void_p(v or 0) if t == "p" else (ctypes.c_int(v) if t == "i" else ctypes.c_float(v)))
    return getattr(_lib.load(), name)(*args, ctypes.c_void_p(0))
