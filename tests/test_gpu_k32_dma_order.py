"""Ring timing of the K = 32 fp16x3 INFERENCE launches (csrc/conv_mfma_k32.hip, the LDS-DMA weight ring): the requests of
weight slab s + 2 are issued piece by piece in the middle of step s, so what can break is a slab read before it landed, a
slab overwritten while still read, or a request that leaves its slab.  None of that depends on the image size; it depends on
the STEP PATTERN, so the cases are the smallest shapes that walk every pattern of every inference instantiation:

  tsr_conv2d_fwd_f16s            3x3 / 5x5, C_out 64 / 128, C_in 16 (phantom block; 3x3: S = 9 steps, ring wrap and almost no
                                 steady state), 32 (one block pair, no next-block halo load), 48 (odd block count after a
                                 pair), 64 (the steps with a halo load in flight)
  tsr_conv2d_fwd_f16s_fuse1x1    3x3 (double-buffered halo) / 5x5, C_in 64 (two block pairs: first pair, a halo load for a
                                 following pair, the tail whose requests fall off the stream), with and without the residual
  tsr_conv2d_fwd_f16s_pair       C_in 32 / 64: alternating half- and full-size slabs

at 8x8 (one tile) and 16x24 (six tiles), B = 1 (absent image slots) and B = 3 (odd image count, a partial workgroup); the
plain launches at 8x8 with B = 1 and 16x24 with B = 3.

Every case runs three times on one set of buffers: with the weight stream in a buffer of exactly its size, with the stream
FOLLOWED IN MEMORY BY NaN (a request that runs past the stream poisons the accumulators), and the second launch once more
immediately.  All three must meet the project's bar per image (tests/_infer_f16s.py: max|got - ref| / max|ref| < 1e-5 against
fp64 on the fp32 operands, inputs randn * 3, per-image maxima within 4x), and all three must agree BIT FOR BIT: a slab race
shows up as a run-to-run difference before it shows up as error.
"""
import pytest
import torch

import _infer_f16s as S
from _infer_f16s import TOL, F16S_SIG, PAIR_SIG, FUSE_SIG
from test_gpu_infer_fp16x3 import f16s_args, pair_args, fuse_args, launch

pytestmark = pytest.mark.gpu

SPATIAL = [(1, 8, 8), (3, 16, 24)]     # the plain launches: (B, H, W)
SIZES = [(8, 8), (16, 24)]             # fuse1x1 and pair: B in {1, 3} at both sizes
OFFS = (16, 32, 48)
POISON = 1 << 16                       # fp16 elements of NaN behind the stream: 128 KB = 8 full slabs

PLAIN = [S.F16sCase(ks, cin, cout, B, H, W, False, False, False, 0, None, OFFS)
         for ks in (3, 5) for cout in (64, 128) for cin in (16, 32, 48, 64) for B, H, W in SPATIAL]
FUSE = [S.FuseCase(ks, 64, B, H, W, 0, False, False, False, res, 0, None, OFFS)
        for ks in (3, 5) for B in (1, 3) for H, W in SIZES for res in (False, True)]
PAIR = [S.PairCase(cin, B, H, W, False, False, 0, None, OFFS[:2]) for cin in (32, 64) for B in (1, 3) for H, W in SIZES]


def k32_elems(cout, cin, ks):
    """fp16 elements of the K = 32 kernel's stream: 2 planes, channel blocks in pairs (tsr_conv_weight_bf16s_elems may
    allot more: it also covers the 32x32x16 kernel's layout)."""
    return 2 * cout * ((cin + 31) & ~31) * ks * ks


def poisoned(wp, n):
    """The first n elements of the packed stream at the head of a larger buffer whose tail is NaN -> (stream, buffer)."""
    assert n <= wp.numel()
    big = torch.full((n + POISON,), float("nan"), dtype=wp.dtype, device=wp.device)
    big[:n] = wp[:n]
    return big[:n], big


def three_runs(name, sig, args, width, wp_plain, wp_poisoned):
    outs = []
    for wp in (wp_plain, wp_poisoned, wp_poisoned):
        args["w_packed"] = wp
        args["out"].fill_(float("nan"))
        launch(name, sig, args)
        outs.append(S.read_slice(args["out"], args["B"], width, args["H"], args["W"], args["out_coff"])[0])
    return outs


def check(tag, c, ref, outs):
    assert S.image_ratio(ref) < 4
    for i, got in enumerate(outs):
        per = S.check_images(got, ref, TOL)
        print(f"[{tag}] {S.cid(c)} run {i}: {S.fmt_images(per)}")
    assert torch.equal(outs[0], outs[1]), "the NaN region behind the weight stream changed the output"
    assert torch.equal(outs[1], outs[2]), "two consecutive launches differ"


@pytest.mark.parametrize("case", PLAIN, ids=S.cid)
def test_plain(case):
    p = S.f16s_inputs(case)
    packed = S.pack_f16s(p["w"])
    n = k32_elems(case.cout, case.cin, case.ks)
    wpp, keep = poisoned(packed[0], n)
    a = f16s_args(p, case.offs, packed=packed)
    check("k32 plain", case, S.f16s_ref(p), three_runs("tsr_conv2d_fwd_f16s", F16S_SIG, a, case.cout, packed[0], wpp))
    assert bool(torch.isnan(keep[n:]).all())


@pytest.mark.parametrize("case", FUSE, ids=S.cid)
def test_fuse1x1(case):
    p = S.fuse_inputs(case)
    packed = S.pack_f16s(p["w"])
    n = k32_elems(128, case.cin, case.ks)
    wpp, keep = poisoned(packed[0], n)
    a = fuse_args(p, case.offs, packed=packed)
    check("k32 fuse1x1", case, S.fuse_ref(p), three_runs("tsr_conv2d_fwd_f16s_fuse1x1", FUSE_SIG, a, 64, packed[0], wpp))
    assert bool(torch.isnan(keep[n:]).all())


@pytest.mark.parametrize("case", PAIR, ids=S.cid)
def test_pair(case):
    p = S.pair_inputs(case)
    packed = S.pack_pair(p["w3"], p["w5"])
    n = packed[0].numel()
    wpp, keep = poisoned(packed[0], n)
    a = pair_args(p, case.offs, packed=packed)
    check("k32 pair", case, S.pair_ref(p), three_runs("tsr_conv2d_fwd_f16s_pair", PAIR_SIG, a, 128, packed[0], wpp))
    assert bool(torch.isnan(keep[n:]).all())
