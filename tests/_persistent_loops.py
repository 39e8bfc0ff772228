"""Case tables, launcher arithmetic and fp64 references of tests/test_gpu_persistent_loops.py -- everything that runs without
a GPU, so that tests/test_persistent_loops_cpu.py can check that the case set reaches the loops it claims to reach.

Four kernel families cap their grid and let a workgroup walk a range of work items.  The caps, quoted from their source:

    fwd1x1_b16k_kernel          csrc/conv1x1_b16k.hip       `const int grid = (int)(total < 512 ? total : 512);`
                                                            `const int per = (int)((total + grid - 1) / grid);`
    dgrad1x1_b16k_kernel<4>     csrc/conv1x1_b16k.hip       `return (int)(groups < 2048 ? groups : 2048);`
                                                            `const int per = (int)(((long long)a.B * gpi + grid - 1) / grid);`
    conv1x1_b16_ex_kernel<64>   csrc/conv_mfma_split16.hip  `dim3(total < 512 ? total : 512)`, `for (t = blockIdx.x; t < total; t += gridDim.x)`
    tpsf_fwd_mfma_kernel        csrc/tpsf_mfma.hip          `grid = B < 256 * TPSF_FWD_OCC ? B : 256 * TPSF_FWD_OCC`, TPSF_FWD_OCC 2
    tpsf_bwd_dhb_kernel         csrc/tpsf_mfma.hip          `grid = B < 256 * TPSF_BWD_OCC ? B : 256 * TPSF_BWD_OCC`, TPSF_BWD_OCC 1
    tpsf_bwd_pool_kernel        csrc/tpsf_mfma.hip          `dim3(B < 2048 ? B : 2048)`
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from test_gpu_conv_ex import q16, fma32

FWD1X1_CAP, DGRAD1X1_CAP, STREAM1X1_CAP = 512, 2048, 512
TPSF_FWD_GRID, TPSF_DHB_GRID, TPSF_POOL_GRID = 512, 256, 2048
FWD1X1_ITEM_PX, FWD1X1_RING, FWD1X1_LOOKAHEAD = 32, 4, 3        # pixels of an item, LDS slots, items requested ahead
DGRAD1X1_GROUP_PX, DGRAD1X1_U = 16, 4                           # pixels of a group, groups in flight
COUT = 64                                                       # forward launches: 256 (128) -> 64
DG_K, DG_N, DG_CIN = 64, 128, 256                               # dgrad launches: K = 64, N = 128 channels of a 256-channel conv


def split(total, cap):
    """(grid, per) of a launch that hands each workgroup `per` consecutive items."""
    grid = min(total, cap)
    return grid, -(-total // grid)


def image_scale(B):
    """2^((b % 7) - 3) per image: consecutive images differ by a factor, exactly representable in bf16."""
    return torch.pow(2.0, (torch.arange(B) % 7 - 3).float()).view(B, 1, 1, 1)


# ------------------------------------------------------------------------------------------- 1. fwd1x1_b16k (nsplit = -3)
# total / per are the issue's columns; the CPU test recomputes them from the launcher's arithmetic
FwdCase = namedtuple("FwdCase", "H W B cin res relu in_coff out_coff res_coff total per")
FWD1X1_CASES = [
    FwdCase(5, 7, 257, 256, None, 1, 16, 32, 0, 514, 2),            # fewer items than the look-ahead; 255 empty workgroups
    FwdCase(5, 7, 513, 256, "plain", 1, 32, 16, 32, 1026, 3),       # = look-ahead; ranges start mid-image
    FwdCase(5, 7, 769, 256, "virtual", 1, 16, 16, 16, 1538, 4),     # = ring size; last range 2 items
    FwdCase(5, 7, 1025, 256, "plain", 0, 32, 32, 16, 2050, 5),      # first slot reuse
    FwdCase(5, 7, 2049, 256, "virtual", 1, 16, 32, 32, 4098, 9),    # two wraps; last non-empty range 3 items
    FwdCase(8, 8, 1025, 256, None, 1, 32, 16, 0, 2050, 5),          # no ragged item
    FwdCase(5, 3, 2561, 256, "plain", 1, 16, 16, 32, 2561, 6),      # every item ragged, every item a new image
    FwdCase(3, 11, 1300, 128, "virtual", 1, 32, 32, 16, 2600, 6),   # C_in 128: fwd1x1_b16k_kernel<8>; 2nd item 1 pixel
]

# ------------------------------------------------------------------------------------------- 3. conv1x1_b16_ex (nsplit = -1)
# virt: virtual input + plain residual, or plain input and no residual
STREAM1X1_CASES = [
    FwdCase(5, 7, 2049, 256, "plain", 1, 16, 32, 16, 513, None),    # 1 tile; workgroup 0 takes two items; last group 1 image
    FwdCase(5, 7, 2049, 256, None, 1, 32, 16, 0, 513, None),
    FwdCase(9, 7, 1030, 256, "plain", 1, 32, 32, 32, 516, None),    # 2 tiles
    FwdCase(9, 7, 1030, 256, None, 1, 16, 16, 0, 516, None),
]


def case_id(c):
    return "-".join("x" if v is None else str(v) for v in c)


def fwd_inputs(c, virtual=True):
    """Operands (bf16-representable where they are stored as bf16) and the fp64 reference of a 1x1 forward, epi_mode 0:
    out = act(W . a + bias + res), a = bf16(relu(fma32(z, s, t))) for a virtual input, a = z for a plain one."""
    g = torch.Generator().manual_seed(5000 + c.B + c.H * 31 + c.W + c.cin)
    sc = image_scale(c.B)
    z = q16(torch.randn(c.B, c.cin, c.H, c.W, generator=g)) * sc
    w = torch.randn(COUT, c.cin, 1, 1, generator=g) * 0.08
    s = torch.rand(c.cin, generator=g) + 0.5 if virtual else None
    t = torch.randn(c.cin, generator=g) * 0.3 if virtual else None
    bias = torch.randn(COUT, generator=g) * 0.1
    r = q16(torch.randn(c.B, COUT, c.H, c.W, generator=g)) * sc
    rs, rt = torch.rand(COUT, generator=g) + 0.5, torch.randn(COUT, generator=g) * 0.3
    a = q16(F.relu(fma32(z, s, t))) if virtual else z
    ref = (a.double().permute(0, 2, 3, 1) @ q16(w).double().view(COUT, c.cin).t()).permute(0, 3, 1, 2)
    ref = ref + bias.double().view(1, -1, 1, 1)
    if c.res == "virtual":
        ref = ref + F.relu(fma32(r, rs, rt)).double()
    elif c.res:
        ref = ref + r.double()
    ref = F.relu(ref) if c.relu else ref
    return dict(z=z, w=w, s=s, t=t, bias=bias, r=r, rs=rs, rt=rt, ref=ref.contiguous())


def swap_item_for_predecessor(out, item, ipi):
    """`out` (B, C, H, W) with the 32-pixel work item `item` (flattened as (image, item of the image)) replaced by the values
    of item - 1: what a ring that serves a step from the slot before the right one would write."""
    B, C, H, W = out.shape
    flat = out.reshape(B, C, H * W).clone()
    (b, q), (pb, pq) = divmod(item, ipi), divmod(item - 1, ipi)
    n = min(FWD1X1_ITEM_PX, H * W - q * FWD1X1_ITEM_PX)
    src = flat[pb, :, pq * FWD1X1_ITEM_PX:pq * FWD1X1_ITEM_PX + n]
    flat[b, :, q * FWD1X1_ITEM_PX:q * FWD1X1_ITEM_PX + src.shape[1]] = src
    return flat.view(B, C, H, W)


# ------------------------------------------------------------------------------------------- 2. dgrad1x1_b16k (nsplit = -3)
DgradCase = namedtuple("DgradCase", "H W B ci0 dz_coff out_coff mask_coff also_without_bn total per")
DGRAD1X1_CASES = [
    DgradCase(5, 7, 683, 0, 16, 32, 16, False, 2049, 2),            # half a U block; 1023 empty workgroups
    DgradCase(5, 7, 1366, 128, 32, 16, 32, False, 4098, 3),
    DgradCase(5, 7, 2731, 0, 16, 16, 32, True, 8193, 5),            # one full U block + 1
    DgradCase(5, 7, 5462, 128, 32, 32, 16, False, 16386, 9),        # two blocks + 1
    DgradCase(4, 4, 8193, 0, 16, 32, 32, False, 8193, 5),           # every group a new image
]


def dgrad_inputs(c):
    """Operands and fp64 references of the masked 1x1 data gradient: v = [fma32(z, ms, mh) > 0] * conv_transpose(dz, bf16(w))
    over channels ci0 .. ci0 + 128, and xhat = z * ba + bb for the BatchNorm-backward sums.  The kernel's mask decision is the
    sign of a correctly rounded fp32 fma, which is the sign of the exact value: no element is left to the device."""
    g = torch.Generator().manual_seed(6000 + c.B + c.H + c.ci0)
    sc = image_scale(c.B)
    dz = q16(torch.randn(c.B, DG_K, c.H, c.W, generator=g)) * sc
    w = torch.randn(DG_K, DG_CIN, 1, 1, generator=g) * 0.05
    z = q16(torch.randn(c.B, DG_N, c.H, c.W, generator=g))
    ms, mh = torch.rand(DG_N, generator=g) + 0.5, torch.randn(DG_N, generator=g) * 0.3
    ba, bb = torch.rand(DG_N, generator=g) + 0.5, torch.randn(DG_N, generator=g) * 0.2
    wq = q16(w)[:, c.ci0:c.ci0 + DG_N].double().view(DG_K, DG_N)
    x = (dz.double().permute(0, 2, 3, 1) @ wq).permute(0, 3, 1, 2)
    pre = z.double() * ms.double().view(1, -1, 1, 1) + mh.double().view(1, -1, 1, 1)
    assert bool((pre != 0).all())
    v = torch.where(pre > 0, x, torch.zeros_like(x)).contiguous()
    xhat = z.double() * ba.double().view(1, -1, 1, 1) + bb.double().view(1, -1, 1, 1)
    return dict(dz=dz, w=w, z=z, ms=ms, mh=mh, ba=ba, bb=bb, v=v, xhat=xhat)


def entry_sums(t, grid, per):
    """(grid, C) sums of t (B, C, H, W) over the pixel groups [e * per, min((e + 1) * per, total)) of entry e, the groups
    flattened as (image, 16-pixel group of the image); an empty range sums to 0."""
    B, C, H, W = t.shape
    gpi = -(-(H * W) // DGRAD1X1_GROUP_PX)
    flat = F.pad(t.reshape(B, C, H * W), (0, gpi * DGRAD1X1_GROUP_PX - H * W))
    groups = flat.view(B, C, gpi, DGRAD1X1_GROUP_PX).sum(-1).permute(0, 2, 1).reshape(B * gpi, C)
    groups = F.pad(groups, (0, 0, 0, grid * per - B * gpi))
    return groups.view(grid, per, C).sum(1)


# ------------------------------------------------------------------------------------------- 4. tPSFNet
TPSF_B = 2100
TPSF_PLATEAU, TPSF_SIGNED, TPSF_ZERO = 256, 512, 2048
# the fp64 comparison: the issue's twelve, the three special samples of the 300-sample test, and later iterations of every grid
TPSF_INDICES = [0, 255, 256, 511, 512, 513, 767, 768, 1024, 2047, 2048, 2099,
                1, 2, 3, 257, 1023, 1025, 1279, 1280, 1536, 1792, 2049, 2098]


def tpsf_inputs():
    """(depth, ab, dLR_deg) drawn as in test_tpsf_kernels_wide_dynamic_range_batch, 2100 DIFFERENT samples; the depth of sample
    b is multiplied by 10^((b % 5) - 2), so that the samples a persistent workgroup handles one after the other (b, b + grid)
    differ by orders of magnitude for each of the grids 512, 256 and 2048 (none is a multiple of 5)."""
    B = TPSF_B
    g = torch.Generator().manual_seed(5)
    depth = torch.rand(B, 100, 100, generator=g) * 10
    depth[1] = depth[1] * 1e-3
    depth[2] = (depth[2] - 5) * 40                  # signed, large
    depth[3] = 0
    depth[3, 40:60, 40:60] = 7.5                    # a real plateau
    ab = torch.rand(B, 3, generator=g) * torch.tensor([1.0, 3.0, 2.0]) + torch.tensor([0.2, 0.25, 0.6])
    dl = torch.randn(B, 16, generator=g)
    depth[TPSF_PLATEAU] = 0
    depth[TPSF_PLATEAU, 30:55, 45:70] = 7.5
    depth[TPSF_SIGNED] = (depth[TPSF_SIGNED] - 5) * 40
    depth[TPSF_ZERO] = 0
    depth = depth * torch.pow(10.0, (torch.arange(B) % 5 - 2).double()).float().view(B, 1, 1)
    return depth, ab, dl
