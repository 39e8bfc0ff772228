"""Case tables, fp64 references, slab checkers and the REFUSAL TABLE of the `tsr_conv2d_ex` tests -- everything that runs
without a GPU (tests/test_conv_ex_cases_cpu.py checks the tables, the references and the checkers, and sends the refusal table
to the library with fake pointers).  tests/test_gpu_conv_ex.py runs the three old tables in the arithmetics of
`TRAIN_IMPLS`; tests/test_gpu_conv_ex_b16k.py runs them, the rows below and the refusal table on the device with the
arithmetic "b16k": nsplit = NS_B16K (-3; NS_B16K_PAIR = -4 for the stage-1 pair), the launches of csrc/conv_b16k.hip and
csrc/conv1x1_b16k.hip that the bf16-storage train step uses for the network's own shapes.

`b16k_accepts(kind, row)` restates when the library takes -3 for a row (a virtual input of a 3x3 / 5x5 launch is first
materialised with tsr_bn_relu_b16, as TrainEngine._plain does; a 1x1 forward keeps it virtual):

    fwd1  (epi_mode 1)   ks in {3, 5}, C_out in {64, 128}, C_in % 32 == 0
    fwd0  (epi_mode 0)   the same shapes with no VIRTUAL residual; or ks = 1, C_out 64, C_in in {128, 256}, virtual input, no scale
    dgrad                ks in {3, 5}: N in {64, 128}, K % 32 == 0 (masked or partial);
                         ks = 1: N = 128, K = 64, masked, no res, no scale
    pair  (-4)           always (C_in % 32 == 0 in every row)

Rows added for the b16k kernels (each also runs nowhere else; nothing above B = 70 or 40x40):

  B16K_FWD1_CASES (row format of FWD1_CASES)
    3x3  32->128 B=1   5x3  plain       | ONE K step, less than one tile, three absent image slots
    5x5  32-> 64 B=5   1x1  virtual     | image smaller than the halo; the second group has three absent slots
    5x5  96->128 B=6  13x21 plain       | odd K-step count, ragged on both axes, two absent slots
  PAIR_CASES (C_in, B, H, W, virtual, in_coff, out_coff)
    32->64|64  B=1   1x1                | one K step, image smaller than the halo
    96->64|64  B=5  13x21 virtual       | odd K-step count, ragged, materialised input
    64->64|64  B=70 12x12               | 18 groups x 4 tiles = 72 workgroups
  B16K_FWD0_CASES (row format of FWD0_CASES)
    3x3 128->128 B=3  9x17 plain in, plain res, scale + shift, no ReLU  | the head's first conv / ResBlock tail shape class
    1x1 128-> 64 B=1  1x1  virtual in, no res, ReLU                     | fwd1x1_b16k_kernel<8>, one ragged item (64 outputs)
    1x1 256-> 64 B=3  5x3  virtual in, VIRTUAL res, ReLU                | every item ragged
  B16K_DGRAD_CASES (row format of DGRAD_CASES)
    5x5 K= 32 N= 64 ci0=64  B=5  1x1  res, scale, mask + sums            | one K step, image smaller than the halo
    3x3 K= 96 N=128 ci0=0   B=6 13x21 res, mask + sums                   | res, mask and out at different ctot AND coff
    1x1 K= 64 N=128 ci0=128 B=3  5x3  mask + sums                        | a ragged last pixel group in every image
    3x3 K= 64 N= 64 ci0=0   B=2  9x17 res, scale, mask, NO bn_a          | the slab's NaN pre-fill survives
    1x1 K= 64 N=128 ci0=0   B=5  4x4  mask, NO bn_a                      | the same on the streaming kernel

Buffers of the b16k harness: `in` is PADS["in"] = 48 channels wider than its slice, `out` 64, `res` 80, `mask` 96 -- the four
tensors of a launch never share a ctot -- and everything outside a slice is NaN.

Bars of "b16k": the project's own for bf16 storage (`check_tensor` with ns = -1, TOL[-1], SUM_TOL[-1]).

The refusal table (`MUTATIONS`, the end of this file): `BASES` holds one small valid launch per arithmetic and epi_mode (B = 1,
5x3, 3x3 32 -> 64; the pair; the two 1x1 forms of -3), every mutation is (name, field changes, bases it applies to) and must
come back as status 1 with nothing launched.
"""
import ctypes
import math

import torch
import torch.nn.functional as F

NAN = float("nan")
NS_B16K, NS_B16K_PAIR = -3, -4
IMPLS = {"f32": 0, "bf16x6": 3, "fp16x3": -2, "bf16op": 1, "bf16x3": 2, "bf16": -1}
TOL = {0: 1e-5, 3: 1e-5, -2: 1e-5, 1: 1e-5, 2: 1e-4, -1: 1e-5}          # outputs (fp32 tensors) and Welford statistics
SUM_TOL = {0: 1e-5, 3: 1e-5, -2: 1e-5, 1: 1e-5, 2: 1e-4, -1: 1e-4}      # BatchNorm-backward sums
GUARD = 8                                                               # NaN entries behind the slab's last entry
PADS = {"in": 48, "out": 64, "res": 80, "mask": 96}


# ---------------------------------------------------------------------------------------------------------------- plumbing
def q16(t):
    return t.bfloat16().float()


def fma32(x, s, t):
    """fp32 fma(x, s_c, t_c) per channel, as the kernels form a virtual input: the product is exact in fp64."""
    return (x.double() * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)).float()


def relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def images_per_workgroup(ns, ks):
    """include/tactilesr_hip.h, tsr_conv2d_slab_entries_ex: 4 for the 3x3 / 5x5 launches of fp16x3 and of the one-plane bf16
    forms (bf16op, bf16 storage, conv_b16k), 2 for everything else."""
    return 4 if ks > 1 and ns in (-2, 1, -1, NS_B16K, NS_B16K_PAIR) else 2


def ref_arith(ns):
    """The arithmetic whose reference and bars a launch of `ns` is held to: conv_b16k is bf16 storage."""
    return -1 if ns in (NS_B16K, NS_B16K_PAIR) else ns


def operands(ns, z, w, s=None, t=None):
    """(stored input, fp64 activation the MFMA sees, fp64 weight the MFMA sees) for arithmetic `ns`."""
    zs = q16(z) if ns == -1 else z
    a = F.relu(fma32(zs, s, t)) if s is not None else zs
    if ns in (1, -1):
        return zs, q16(a).double(), q16(w).double()
    return zs, a.double(), w.double()


def check_tensor(ns, got, ref):
    """The bar of arithmetic `ns` on one output tensor (got fp32 values, ref fp64); returns the figures as text."""
    assert torch.isfinite(got).all()
    if ns == -1:
        r16 = q16(ref.float())
        d = (got - r16).abs()
        same = float((d == 0).float().mean())
        bad = d > torch.maximum(1.01 * r16.abs() * 2.0 ** -7, torch.full_like(r16, 3e-6 * float(r16.abs().max())))
        txt = f"identical {same:.5f}, beyond one ulp {int(bad.sum())}"
        assert not bad.any(), txt
        if got.numel() >= 100:
            assert same >= 0.99, txt
        return txt
    e = relerr(got, ref)
    assert e < TOL[ns], e
    return f"{e:.1e}"


def _cv(v):
    return v.double().view(1, -1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- slabs
def entry_counts(img, B, H, W):
    """(entries, expected valid-pixel count of every entry) of a tiled launch with `img` images per workgroup: entry
    (image group * tiles + tile) * img + slot holds image group * img + slot."""
    ty, tx = (H + 7) // 8, (W + 7) // 8
    groups = (B + img - 1) // img
    rows = torch.tensor([min(8, H - 8 * i) for i in range(ty)], dtype=torch.float64)
    cols = torch.tensor([min(8, W - 8 * i) for i in range(tx)], dtype=torch.float64)
    px = (rows[:, None] * cols[None, :]).reshape(1, -1, 1)
    present = (torch.arange(groups * img) < B).double().view(groups, 1, img)
    return groups * ty * tx * img, (px * present).reshape(-1)


def entry_image_tile(e, img, B, H, W):
    """(image, y0, x0) of entry e; image >= B: an absent slot."""
    tx_n, tiles = (W + 7) // 8, ((H + 7) // 8) * ((W + 7) // 8)
    b, t = (e // (tiles * img)) * img + e % img, (e // img) % tiles
    return b, (t // tx_n) * 8, (t % tx_n) * 8


def check_welford_host(slab, cnt, ref, img, tol, check_var=True):
    """epi_mode 1 slabs (cpu tensors of entries + GUARD entries) against the fp64 output `ref`: guard band, counts, per-entry
    means, Chan-merged mean / variance."""
    B, cout, H, W = ref.shape
    entries, want_cnt = entry_counts(img, B, H, W)
    sl = slab.double().view(entries + GUARD, cout, 2)
    n_e = cnt.double()
    assert torch.isnan(sl[entries:]).all() and torch.isnan(n_e[entries:]).all(), "an entry was written out of range"
    assert torch.isfinite(sl[:entries]).all() and torch.isfinite(n_e[:entries]).all(), "an entry was not written"
    sl, n_e = sl[:entries], n_e[:entries]
    assert torch.equal(n_e, want_cnt), "per-entry valid-pixel counts"
    assert float(n_e.sum()) == B * H * W
    scale = float(ref.abs().max())
    e_ent = 0.0
    for e in range(entries):
        b, y0, x0 = entry_image_tile(e, img, B, H, W)
        if b >= B:
            assert float(sl[e].abs().max()) == 0.0          # an absent image: count 0, mean 0, M2 0
            continue
        e_ent = max(e_ent, float((sl[e, :, 0] - ref[b, :, y0:y0 + 8, x0:x0 + 8].mean(dim=(1, 2))).abs().max()) / scale)
    N = float(n_e.sum())
    mean = (sl[:, :, 0] * n_e[:, None]).sum(0) / N
    m2 = (sl[:, :, 1] + n_e[:, None] * (sl[:, :, 0] - mean[None]) ** 2).sum(0)
    rm, rv = ref.mean(dim=(0, 2, 3)), ref.var(dim=(0, 2, 3), unbiased=False)
    e_m = float((mean - rm).abs().max()) / scale
    if float(rv.max()) > 0:
        e_v = float((m2 / N - rv).abs().max() / rv.max())
    else:                                                   # ONE pixel in all: the variance is zero and M2 must be exactly 0
        e_v = 0.0 if float(m2.abs().max()) == 0.0 else float("inf")
    assert e_ent < tol and e_m < tol and (e_v < tol or not check_var), (e_ent, e_m, e_v)
    return f"entry means {e_ent:.1e}, mean {e_m:.1e}, var {e_v:.1e}"


def tiled_entry_sums(x, xhat, img):
    """(entries, C, 2): sum(x), sum(x * xhat) over the valid pixels of every entry of a tiled launch; absent slots 0."""
    B, C, H, W = x.shape
    entries, _ = entry_counts(img, B, H, W)
    out = torch.zeros(entries, C, 2, dtype=torch.float64)
    for e in range(entries):
        b, y0, x0 = entry_image_tile(e, img, B, H, W)
        if b < B:
            xs, hs = x[b, :, y0:y0 + 8, x0:x0 + 8], xhat[b, :, y0:y0 + 8, x0:x0 + 8]
            out[e, :, 0], out[e, :, 1] = xs.sum(dim=(1, 2)), (xs * hs).sum(dim=(1, 2))
    return out


def dgrad1x1_split(B, H, W):
    """(grid = entries, pixel groups per workgroup) of dgrad1x1_b16k_kernel (csrc/conv1x1_b16k.hip; tests/_persistent_loops.py)."""
    total = B * -(-(H * W) // 16)
    grid = min(total, 2048)
    return grid, -(-total // grid)


def streamed_entry_sums(x, xhat, grid, per):
    """(grid, C, 2): the same sums over workgroup e's contiguous range [e * per, (e + 1) * per) of 16-pixel groups, the groups
    flattened as (image, group of the image) (tests/_persistent_loops.py: entry_sums)."""
    def one(t):
        B, C, H, W = t.shape
        gpi = -(-(H * W) // 16)
        flat = F.pad(t.reshape(B, C, H * W), (0, gpi * 16 - H * W))
        groups = flat.view(B, C, gpi, 16).sum(-1).permute(0, 2, 1).reshape(B * gpi, C)
        return F.pad(groups, (0, 0, 0, grid * per - B * gpi)).view(grid, per, C).sum(1)
    return torch.stack([one(x), one(x * xhat)], -1)


def check_dgrad_sums_host(slab, want, tol):
    """epi_mode 2 slab (cpu tensor of entries + GUARD entries) against the per-entry fp64 sums `want` (entries, C, 2): guard
    band, every entry written, every entry's two sums (relative to the largest entry sum of its kind), the sums over all
    entries (relative to the largest channel sum)."""
    entries, C, _ = want.shape
    sl = slab.double().view(entries + GUARD, C, 2)
    assert torch.isnan(sl[entries:]).all(), "an entry was written out of range"
    assert torch.isfinite(sl[:entries]).all(), "an entry was not written"
    sl = sl[:entries]
    ee = [relerr(sl[:, :, k], want[:, :, k]) for k in (0, 1)]
    et = [relerr(sl[:, :, k].sum(0), want[:, :, k].sum(0)) for k in (0, 1)]
    txt = f"entry sums {ee[0]:.1e} / {ee[1]:.1e}, sums {et[0]:.1e} / {et[1]:.1e}"
    assert max(ee) < tol and max(et) < tol, txt
    return txt


# ---------------------------------------------------------------------------------------------------------------- tables
# (ks, cin, cout, B, H, W, virtual input, in_coff, out_coff, out_amax prior: None = no out_amax)
FWD1_CASES = [
    (3, 64, 64, 3, 40, 40, True, 16, 32, 0.0),
    (5, 128, 128, 2, 13, 21, True, 32, 16, 1.0e6),
    (1, 256, 64, 5, 9, 17, True, 16, 16, None),
    (3, 16, 128, 1, 5, 3, False, 32, 32, 0.0),
    (5, 48, 64, 2, 1, 1, True, 16, 32, None),
    (1, 128, 128, 3, 13, 21, False, 32, 16, 0.0),
    (3, 128, 64, 70, 12, 12, False, 16, 32, None),
    (5, 64, 128, 3, 40, 40, False, 16, 16, 0.0),
    (3, 256, 128, 2, 9, 17, True, 32, 16, None),
    (1, 64, 64, 1, 40, 40, True, 16, 32, 0.0),
]
B16K_FWD1_CASES = [
    (3, 32, 128, 1, 5, 3, False, 16, 32, None),
    (5, 32, 64, 5, 1, 1, True, 32, 16, None),
    (5, 96, 128, 6, 13, 21, False, 16, 16, None),
]

# (ks, cin, cout, B, H, W, virtual input, residual: None / "plain" / "virtual", relu, scale, in_coff, out_coff, res_coff)
FWD0_CASES = [
    (1, 256, 64, 2, 40, 40, True, "plain", 1, False, 16, 32, 16),
    (1, 256, 64, 3, 13, 21, True, "virtual", 1, False, 32, 16, 32),
    (3, 64, 64, 5, 9, 17, False, "plain", 1, False, 16, 32, 0),
    (3, 64, 64, 1, 5, 3, False, None, 1, False, 32, 16, 0),
    (1, 128, 128, 2, 1, 1, True, None, 0, False, 16, 32, 0),
    (5, 48, 128, 3, 13, 21, True, "virtual", 0, True, 32, 16, 32),
    (5, 16, 64, 2, 9, 17, False, "plain", 0, False, 16, 16, 32),
    (1, 64, 64, 70, 12, 12, False, "plain", 1, False, 32, 32, 16),
    (3, 128, 128, 2, 40, 40, True, "plain", 1, False, 16, 32, 32),
]
B16K_FWD0_CASES = [
    (3, 128, 128, 3, 9, 17, False, "plain", 0, True, 16, 32, 48),
    (1, 128, 64, 1, 1, 1, True, None, 1, False, 16, 32, 0),
    (1, 256, 64, 3, 5, 3, True, "virtual", 1, False, 32, 16, 48),
]

# (ks, K = the conv's C_out, cin of the conv, N = nprime, ci0, B, H, W, residual, form, scale,
#  dz_coff, out_coff, res_coff, mask_coff);  form: "bn" = epi_mode 2 + sums, "mask" = epi_mode 2 without bn_a,
#  "partial" = epi_mode 0 without a mask
DGRAD_CASES = [
    (3, 64, 64, 64, 0, 3, 40, 40, True, "bn", False, 16, 32, 16, 32),
    (5, 128, 192, 128, 64, 2, 13, 21, True, "bn", True, 32, 16, 32, 16),
    (1, 64, 256, 128, 128, 5, 9, 17, False, "bn", False, 16, 16, 0, 32),
    (3, 16, 64, 64, 0, 1, 5, 3, True, "bn", False, 32, 32, 16, 16),
    (5, 48, 128, 64, 64, 2, 1, 1, True, "mask", False, 16, 32, 32, 16),
    (1, 256, 64, 64, 0, 3, 13, 21, False, "partial", True, 32, 16, 0, 0),
    (3, 128, 128, 128, 0, 70, 12, 12, True, "bn", False, 16, 32, 32, 16),
    (5, 64, 64, 64, 0, 3, 40, 40, True, "partial", False, 16, 16, 32, 0),
    (3, 256, 128, 128, 0, 2, 9, 17, True, "bn", False, 32, 16, 0, 48),
    (1, 128, 128, 64, 64, 1, 40, 40, True, "bn", False, 16, 32, 16, 32),
]
B16K_DGRAD_CASES = [
    (5, 32, 128, 64, 64, 5, 1, 1, True, "bn", True, 16, 32, 16, 48),
    (3, 96, 128, 128, 0, 6, 13, 21, True, "bn", False, 32, 16, 48, 0),
    (1, 64, 256, 128, 128, 3, 5, 3, False, "bn", False, 16, 32, 0, 48),
    (3, 64, 64, 64, 0, 2, 9, 17, True, "mask", True, 16, 16, 32, 48),
    (1, 64, 128, 128, 0, 5, 4, 4, False, "mask", False, 32, 16, 0, 32),
]

# (cin, B, H, W, virtual input, in_coff, out_coff): conv_3_1 || conv_5_1 -> 64 | 64 channels, epi_mode 1
PAIR_CASES = [
    (32, 1, 1, 1, False, 16, 32),
    (96, 5, 13, 21, True, 32, 16),
    (64, 70, 12, 12, False, 16, 48),
]

TABLES = {"fwd1": FWD1_CASES + B16K_FWD1_CASES, "fwd0": FWD0_CASES + B16K_FWD0_CASES, "dgrad": DGRAD_CASES + B16K_DGRAD_CASES,
          "pair": PAIR_CASES}


def cid(c):
    return "-".join("x" if v is None else str(v) for v in c)


def b16k_accepts(kind, row):
    """Whether tsr_conv2d_ex takes nsplit = -3 (-4 for `pair`) for this row (see the module docstring)."""
    if kind == "pair":
        return row[0] % 32 == 0
    if kind == "fwd1":
        ks, cin, cout = row[:3]
        return ks in (3, 5) and cout in (64, 128) and cin % 32 == 0
    if kind == "fwd0":
        ks, cin, cout, _, _, _, virt, res, _, use_scale = row[:10]
        if ks in (3, 5):
            return cout in (64, 128) and cin % 32 == 0 and res != "virtual"
        return ks == 1 and cout == 64 and cin in (128, 256) and virt and not use_scale
    ks, K, _, NP, _, _, _, _, use_res, form, use_scale = row[:11]
    if ks in (3, 5):
        return NP in (64, 128) and K % 32 == 0
    return ks == 1 and NP == 128 and K == 64 and form != "partial" and not use_res and not use_scale


# ---------------------------------------------------------------------------------------------------------------- problems
def make_problem(kind, row, ns=-1):
    """CPU operands, descriptor integers and the fp64 reference of one row for the reference arithmetic `ns` (ref_arith of
    the launch's nsplit).  Keys: ks cin cout B H W epi relu; z (stored input) s t (virtual input or None); wkind ("fwd" /
    "dgrad" / "pair") and w (OIHW; dgrad: the forward conv's weight with ci0 / cin_f; pair: w3 w5); scale shift; r rs rt
    (residual); mz ms mh ba bb bn (mask); coff {in, out, res, mask}; prior (out_amax); ref = the expected output in fp64 --
    for a masked dgrad the UNMASKED x and `pre`, the mask pre-activation (see dgrad_expected)."""
    P = dict(kind=kind, row=row, s=None, t=None, scale=None, shift=None, r=None, rs=None, rt=None, mz=None, bn=False, relu=0,
             prior=None, wkind="fwd", coff={})
    if kind == "fwd1":
        ks, cin, cout, B, H, W, virt, in_coff, out_coff, prior = row
        g = torch.Generator().manual_seed(1000 + ks * 7 + cin + cout + B + H)
        z = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
        if virt:
            P["s"], P["t"] = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
        zs, a, wr = operands(ns, z, w, P["s"], P["t"])
        P.update(epi=1, z=zs, w=w, prior=prior, coff={"in": in_coff, "out": out_coff}, ref=F.conv2d(a, wr, padding=ks // 2))
    elif kind == "pair":
        cin, B, H, W, virt, in_coff, out_coff = row
        ks, cout = 5, 128
        g = torch.Generator().manual_seed(1500 + cin + 7 * B + H)
        z = torch.randn(B, cin, H, W, generator=g)
        w3, w5 = torch.randn(64, cin, 3, 3, generator=g) * 0.08, torch.randn(64, cin, 5, 5, generator=g) * 0.05
        if virt:
            P["s"], P["t"] = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
        w = torch.cat([F.pad(w3, (1, 1, 1, 1)), w5], 0)
        zs, a, wr = operands(ns, z, w, P["s"], P["t"])
        ref = torch.cat([F.conv2d(a, wr[:64, :, 1:4, 1:4], padding=1), F.conv2d(a, wr[64:], padding=2)], 1)
        P.update(epi=1, z=zs, w=w, wkind="pair", coff={"in": in_coff, "out": out_coff}, ref=ref)
    elif kind == "fwd0":
        ks, cin, cout, B, H, W, virt, res, relu, use_scale, in_coff, out_coff, res_coff = row
        g = torch.Generator().manual_seed(2000 + ks * 7 + cin + cout + B + H)
        z = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
        if virt:
            P["s"], P["t"] = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
        scale = torch.rand(cout, generator=g) + 0.5 if use_scale else None
        shift = torch.randn(cout, generator=g) * 0.1
        r = torch.randn(B, cout, H, W, generator=g)
        rs, rt = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
        zs, a, wr = operands(ns, z, w, P["s"], P["t"])
        rq = q16(r) if ns == -1 else r
        ref = F.conv2d(a, wr, padding=ks // 2)
        if use_scale:
            ref = ref * _cv(scale)
        ref = ref + _cv(shift)
        if res == "virtual":
            ref = ref + F.relu(fma32(rq, rs, rt)).double()
            P["rs"], P["rt"] = rs, rt
        elif res:
            ref = ref + rq.double()
        ref = F.relu(ref) if relu else ref
        P.update(epi=0, z=zs, w=w, scale=scale, shift=shift, relu=relu, r=rq if res else None,
                 coff={"in": in_coff, "out": out_coff, "res": res_coff}, ref=ref)
    else:
        ks, K, cin_f, NP, ci0, B, H, W, use_res, form, use_scale, dz_coff, out_coff, res_coff, mask_coff = row
        g = torch.Generator().manual_seed(3000 + ks * 7 + K + cin_f + B + H)
        dz = torch.randn(B, K, H, W, generator=g)
        w = torch.randn(K, cin_f, ks, ks, generator=g) * 0.05
        z = torch.randn(B, NP, H, W, generator=g)
        extra = torch.randn(B, NP, H, W, generator=g) * 0.1
        ms, mh = torch.rand(NP, generator=g) + 0.5, torch.randn(NP, generator=g) * 0.3
        ba, bb = torch.rand(NP, generator=g) + 0.5, torch.randn(NP, generator=g) * 0.2
        scale = torch.rand(NP, generator=g) + 0.5 if use_scale else None
        if ns == -1:
            dz, z, extra = q16(dz), q16(z), q16(extra)
        dzr, wr = (q16(dz), q16(w)) if ns in (1, -1) else (dz, w)
        x = F.conv_transpose2d(dzr.double(), wr[:, ci0:ci0 + NP].double(), padding=ks // 2)
        if use_scale:
            x = x * _cv(scale)
        if use_res:
            x = x + extra.double()
        cin, cout = K, NP
        P.update(epi=0 if form == "partial" else 2, z=dz, w=w, wkind="dgrad", ci0=ci0, cin_f=cin_f, scale=scale,
                 r=extra if use_res else None, coff={"in": dz_coff, "out": out_coff, "res": res_coff, "mask": mask_coff}, ref=x)
        if form != "partial":
            P.update(mz=z, ms=ms, mh=mh, ba=ba, bb=bb, bn=form == "bn", pre=z.double() * _cv(ms) + _cv(mh),
                     xhat=z.double() * _cv(ba) + _cv(bb))
    P.update(ks=ks, cin=cin, cout=cout, B=B, H=H, W=W)
    return P


def dgrad_expected(P, got):
    """(expected output, share of near-zero mask pre-activations) of a masked dgrad: elements whose fp64 pre-activation is
    within 1e-6 of zero (relative to its max) take the decision `got` shows; their share is capped at 1e-4."""
    if P["mz"] is None:
        return P["ref"], 0.0
    pre = P["pre"]
    near = pre.abs() < 1e-6 * pre.abs().max()
    share = float(near.double().mean())
    assert share <= 1e-4
    on = torch.where(near, got != 0, pre > 0)
    return torch.where(on, P["ref"], torch.zeros_like(P["ref"])), share


def near_zero_share(P):
    pre = P["pre"]
    return float((pre.abs() < 1e-6 * pre.abs().max()).double().mean())


def materialised(P):
    """What tsr_bn_relu_b16 must leave of a virtual bf16 input, bit for bit: q16(relu(fma32(q16(z), s, t)))."""
    return q16(F.relu(fma32(q16(P["z"]), P["s"], P["t"])))


# ---------------------------------------------------------------------------------------------------------------- descriptor
PTR_FIELDS = ("in", "w_packed", "scale", "shift", "res", "out", "in_scale", "in_shift", "res_scale", "res_shift", "mask",
              "mask_scale", "mask_shift", "bn_a", "bn_b", "slab", "slab_cnt", "in_amax", "out_amax", "w_amax")
FAKE = 16                               # a non-NULL pointer value that is never dereferenced (the CPU test's)


def desc_ints(P, nsplit, materialise=False):
    """The integer / float fields of the valid descriptor of problem P launched with `nsplit`."""
    d = dict(in_ctot=P["cin"] + PADS["in"], in_coff=P["coff"]["in"], cin=P["cin"], cout=P["cout"], ks=P["ks"],
             out_ctot=P["cout"] + PADS["out"], out_coff=P["coff"]["out"], relu=int(P["relu"]), B=P["B"], H=P["H"], W=P["W"],
             epi_mode=P["epi"], nsplit=nsplit, w_inv_scale=1.0, res_ctot=0, res_coff=0, mask_ctot=0, mask_coff=0)
    if materialise:
        d.update(in_ctot=P["cin"], in_coff=0)
    if P["r"] is not None:
        d.update(res_ctot=P["cout"] + PADS["res"], res_coff=P["coff"]["res"])
    if P["mz"] is not None:
        d.update(mask_ctot=P["cout"] + PADS["mask"], mask_coff=P["coff"]["mask"])
    return d


def desc_ptrs(P, nsplit, materialise=False):
    """Names of the pointer fields the valid descriptor sets (the statistics slabs are ALWAYS handed over: a launch that has
    no use for them must leave their NaN fill alone)."""
    fp32 = ref_arith(nsplit) != -1
    have = {"in", "w_packed", "out", "slab", "slab_cnt"}
    have |= {k for k in ("scale", "shift") if P[k] is not None}
    if P["s"] is not None and not materialise:
        have |= {"in_scale", "in_shift"}
    if P["r"] is not None:
        have |= {"res"} | ({"res_scale", "res_shift"} if P["rs"] is not None else set())
    if P["mz"] is not None:
        have |= {"mask", "mask_scale", "mask_shift"} | ({"bn_a", "bn_b"} if P["bn"] else set())
    if nsplit == -2:
        have |= {"in_amax", "w_amax"}
    if fp32 and (P["epi"] != 1 or P["prior"] is not None):
        have.add("out_amax")
    return have


def fill_desc(vals):
    """A ConvDesc from `vals` (field -> None / int pointer value / tensor / int / float; "in" is the field `in_`)."""
    from tactilesr_amd.model._train import ConvDesc
    types = dict(ConvDesc._fields_)
    d = ConvDesc()
    for k, v in vals.items():
        f = "in_" if k == "in" else k
        if types[f] is ctypes.c_void_p:
            v = None if v is None else (v if isinstance(v, int) else v.data_ptr())
        setattr(d, f, v)
    return d


def raw_ex(vals, stream=None):
    """Status of tsr_conv2d_ex for the descriptor `vals`; `vals` None = a NULL descriptor."""
    from tactilesr_amd import _lib
    d = None if vals is None else ctypes.byref(fill_desc(vals))
    return _lib.load().tsr_conv2d_ex(d, ctypes.c_void_p(0) if stream is None else stream)


# ---------------------------------------------------------------------------------------------------------------- refusals
# One valid launch per arithmetic and epi_mode: (nsplit, kind, row).  B = 1, a 5x3 image, 3x3 32 -> 64 (one K step of conv_b16k,
# two channel blocks of every other kernel); the pair; the two 1x1 forms of -3.
_B0 = (3, 32, 64, 1, 5, 3, False, "plain", 1, True, 16, 32, 48)
_B1 = (3, 32, 64, 1, 5, 3, False, 16, 32, 0.0)
_B2 = (3, 32, 64, 64, 0, 1, 5, 3, True, "bn", True, 16, 32, 48, 16)
ARITH = dict(IMPLS, b16k=NS_B16K)
BASES = {}
for _name, _ns in ARITH.items():
    BASES[f"{_name}/0"], BASES[f"{_name}/1"], BASES[f"{_name}/2"] = (_ns, "fwd0", _B0), (_ns, "fwd1", _B1), (_ns, "dgrad", _B2)
BASES["pair/1"] = (NS_B16K_PAIR, "pair", (32, 1, 5, 3, False, 16, 32))
BASES["b16k1x1f/0"] = (NS_B16K, "fwd0", (1, 128, 64, 1, 5, 3, True, "plain", 1, False, 16, 32, 48))
BASES["b16k1x1d/2"] = (NS_B16K, "dgrad", (1, 64, 128, 128, 0, 1, 5, 3, False, "bn", False, 16, 32, 0, 16))

VEC, BUF = "<vec>", "<buf>"             # pointer values of a mutation: a per-channel fp32 vector / a tensor buffer


def base_problem(key):
    ns, kind, row = BASES[key]
    return make_problem(kind, row, ref_arith(ns))


def fake_desc(key):
    """The valid descriptor of base `key` with the FAKE pointer value in every pointer field it sets."""
    ns = BASES[key][0]
    P = base_problem(key)
    d = desc_ints(P, ns)
    d.update({k: (FAKE if k in desc_ptrs(P, ns) else None) for k in PTR_FIELDS})
    return d


def _keys(arith=None, epi=None):
    """Base keys "<arithmetic>/<epi_mode>" of the arithmetics `arith` (None: all, the pair and 1x1 bases included) and of
    the epi_modes `epi` (None: all)."""
    return tuple(k for k in BASES if (arith is None or k.split("/")[0] in arith) and (epi is None or int(k.split("/")[1]) in epi))


def _mutations():
    ALL = _keys()
    RES = tuple(k for k in _keys(epi=(0, 2)) if k != "b16k1x1d/2")        # bases that hand a residual over
    M = [("d = NULL", None, ALL)]
    M += [(f"{p} = NULL", {p: None}, ALL) for p in ("in", "w_packed", "out")]
    M += [(f"{d} = {v}", {d: v}, ALL) for d in ("B", "H", "W") for v in (0, -1)]
    M += [("cin = 0", {"cin": 0}, ALL), ("cin = -16", {"cin": -16}, ALL), ("cin + 8", {"cin": lambda d: d["cin"] + 8}, ALL),
          ("in_ctot - 8", {"in_ctot": lambda d: d["in_ctot"] - 8}, ALL), ("in_coff = 8", {"in_coff": 8}, ALL),
          ("out_ctot - 8", {"out_ctot": lambda d: d["out_ctot"] - 8}, ALL), ("out_coff = 24", {"out_coff": 24}, ALL),
          ("in_coff = -16", {"in_coff": -16}, ALL), ("out_coff = -16", {"out_coff": -16}, ALL),
          ("in slice leaves its buffer", {"in_coff": lambda d: d["in_ctot"] - d["cin"] + 16}, ALL),
          ("out slice leaves its buffer", {"out_coff": lambda d: d["out_ctot"] - d["cout"] + 16}, ALL),
          ("res_ctot - 8", {"res_ctot": lambda d: d["res_ctot"] - 8}, RES), ("res_coff = 8", {"res_coff": 8}, RES),
          ("res_coff = -16", {"res_coff": -16}, RES),
          ("res slice leaves its buffer", {"res_coff": lambda d: d["res_ctot"] - d["cout"] + 16}, RES)]
    E2 = _keys(epi=(2,))
    M += [("mask_ctot - 8", {"mask_ctot": lambda d: d["mask_ctot"] - 8}, E2), ("mask_coff = 8", {"mask_coff": 8}, E2),
          ("mask_coff = -16", {"mask_coff": -16}, E2),
          ("mask slice leaves its buffer", {"mask_coff": lambda d: d["mask_ctot"] - d["cout"] + 16}, E2),
          ("epi_mode 2 without mask", {"mask": None}, E2), ("bn_a without bn_b", {"bn_b": None}, E2),
          ("bn_a without slab", {"slab": None}, E2)]
    # a width the kernels do not have; the buffers are widened so that only this rule can refuse
    wide = {"out_ctot": 384, "res_ctot": lambda d: d["res_ctot"] and 384, "mask_ctot": lambda d: d["mask_ctot"] and 384}
    M += [(f"cout = {c}", dict(wide, cout=c), ALL) for c in (0, 32, 96, 256)]
    M += [(f"ks = {k}", {"ks": k}, ALL) for k in (-3, 0, 2, 4, 7)]
    M += [("epi_mode = -1", {"epi_mode": -1}, ALL), ("epi_mode = 3", {"epi_mode": 3}, ALL)]
    E1 = _keys(epi=(1,))
    M += [("epi_mode 1 without slab", {"slab": None}, E1), ("epi_mode 1 without slab_cnt", {"slab_cnt": None}, E1)]
    M += [("in_scale without in_shift", {"in_scale": VEC, "in_shift": None}, ALL),
          ("in_shift without in_scale", {"in_scale": None, "in_shift": VEC}, ALL),
          ("res_scale without res_shift", {"res_scale": VEC, "res_shift": None}, ALL),
          ("res_shift without res_scale", {"res_scale": None, "res_shift": VEC}, ALL)]
    M += [("nsplit = -5", {"nsplit": -5}, ALL), ("nsplit = 4", {"nsplit": 4}, ALL)]
    F16 = _keys(arith=("fp16x3",))
    M += [("-2: in_amax = NULL", {"in_amax": None}, F16)]
    M += [(f"-2: w_inv_scale = {v} without w_amax", {"w_amax": None, "w_inv_scale": v}, F16) for v in (0.0, -1.0, NAN)]
    M += [("-1: 1x1 C_out 64 epi_mode 0, C_in 544 (72 KB of LDS)", {"ks": 1, "cin": 544, "in_ctot": 592}, ("bf16/0",))]
    K3 = _keys(arith=("b16k",))
    M += [("-3: virtual input, ks > 1", {"in_scale": VEC, "in_shift": VEC}, K3),
          ("-3: virtual residual, ks > 1", {"res_scale": VEC, "res_shift": VEC}, K3),
          ("-3: C_in 48", {"cin": 48}, K3), ("-3: C_in 16", {"cin": 16}, K3),
          ("-3: 8 * in_ctot * H * W >= 2^31", {"H": 2048, "W": 2048}, K3)]
    M += [("-3: ks = 1, epi_mode 1", {"epi_mode": 1}, ("b16k1x1f/0",)),
          ("-3: ks = 1, epi_mode 0, plain input", {"in_scale": None, "in_shift": None}, ("b16k1x1f/0",)),
          ("-3: ks = 1, epi_mode 0, scale", {"scale": VEC}, ("b16k1x1f/0",)),
          ("-3: ks = 1, epi_mode 0, C_in 64", {"cin": 64}, ("b16k1x1f/0",)),
          ("-3: ks = 1, epi_mode 2, res", {"res": BUF, "res_ctot": 208, "res_coff": 48}, ("b16k1x1d/2",)),
          ("-3: ks = 1, epi_mode 2, scale", {"scale": VEC}, ("b16k1x1d/2",)),
          ("-3: ks = 1, epi_mode 2, N = 64", {"cout": 64}, ("b16k1x1d/2",)),
          ("-3: ks = 1, epi_mode 2, K = 128", {"cin": 128, "in_ctot": 176}, ("b16k1x1d/2",))]
    PR = ("pair/1",)
    M += [("-4: ks = 3", {"ks": 3}, PR), ("-4: cout = 64", {"cout": 64}, PR), ("-4: epi_mode 0", {"epi_mode": 0}, PR),
          ("-4: epi_mode 2", {"epi_mode": 2, "mask": BUF, "mask_ctot": 224, "mask_coff": 16}, PR),
          ("-4: no slab", {"slab": None}, PR), ("-4: virtual input", {"in_scale": VEC, "in_shift": VEC}, PR),
          ("-4: C_in 48", {"cin": 48}, PR)]
    return M


MUTATIONS = _mutations()
CPU_ONLY = ("-3: 8 * in_ctot * H * W >= 2^31",)      # host arithmetic on an image no test buffer holds: fake pointers only


def mutated(base, changes, vec=FAKE, buf=FAKE):
    """`base` (a descriptor dict) with `changes` applied; None = the NULL descriptor.  A callable value is computed from
    the base's fields; VEC / BUF stand for a pointer the caller supplies."""
    if changes is None:
        return None
    d = dict(base)
    for k, v in changes.items():
        if v == VEC:
            v = vec
        elif v == BUF:
            v = buf
        elif callable(v):
            v = v(base)
        d[k] = v
    return d


def mutations_of(key):
    return [(name, ch) for name, ch, keys in MUTATIONS if key in keys]


def is_nan_value(v):
    return isinstance(v, float) and math.isnan(v)
