"""Kernel-level tests of `tsr_conv2d_ex`, ONE LAUNCH AT A TIME, in every arithmetic of the train step.

`tsr_conv2d_ex` is the launch behind every 1x1 / 3x3 / 5x5 convolution of the train step; `tsr_conv_desc.nsplit` picks the
kernel family.  Each test drives one launch through the engine's own helpers (`conv_ex`, `Act`, `_pack`, `_pack_dgrad` of
tactilesr_amd.model._train) and compares EVERY output of that launch with the same operation in fp64 torch on the CPU.  The
whole-network tests cannot say which launch is wrong, and dilute an error confined to one ragged tile, one image slot of a
4-image workgroup or one channel block of an offset slice; these can.

Arithmetics (nsplit), kernels, images per workgroup (= statistics-slab entries per workgroup):

    f32     0   conv_mfma_f32.hip                                                    2
    bf16x6  3   conv_mfma_split16.hip NS = 3 (3x3: double-buffered halo if C_in/16 even)   2
    bf16x3  2   conv_mfma_split16.hip NS = 2 (reduced precision: 1e-4)               2
    bf16op  1   conv_mfma_split16.hip NS = 1                                         4 (3x3 / 5x5), 2 (1x1)
    fp16x3 -2   conv_mfma_k32.hip (3x3 / 5x5: C_out 64 = 256 threads, 128 = 512)     4
                conv_mfma_split16.hip (1x1)                                          2
    bf16   -1   conv_mfma_split16.hip IO16 (3x3 / 5x5)                               4
                IO16 1x1 tiled (C_out 128, or any launch with slabs)                 2
                conv1x1_b16_ex_kernel (1x1, C_out 64, epi_mode 0: streaming)         4 (no slabs)
    b16k   -3   conv_b16k.hip TRAIN / DGRAD / PLAIN (3x3 / 5x5, C_in % 32 == 0)      4     tests/test_gpu_conv_ex_b16k.py: these
           -4   conv_b16k.hip PAIR_TRAIN (the stage-1 pair, 5x5 -> 64 | 64)          4     tables, more rows and the refusal
           -3   conv1x1_b16k.hip (1x1: virtual-input forward 128 / 256 -> 64,        1 entry per workgroup (masked dgrad)
                masked dgrad 64 -> 128)                                                    matrix of tsr_conv2d_ex

The tables, the pure helpers and the fp64 references live in tests/_conv_ex_cases.py (checked without a device by
tests/test_conv_ex_cases_cpu.py).

Case lists -- hand-picked against the tiling (8x8 pixel tiles; 2 or 4 images per workgroup; channel blocks of 16 paired into
K = 32 steps), every row runs with EVERY arithmetic.  `K` is the launch's reduction width (C_in of a forward, the conv's
C_out of a data gradient), `N` its output width; offsets are (input, output, residual, mask) channel offsets inside buffers
that are 48 channels wider than the slice, everything outside the slices is NaN:

  forward, epi_mode 1 (FWD1_CASES)              | why
    3x3  64-> 64 B=3 40x40 virtual              | network shape; B not a multiple of 2 / 4: one absent image slot
    5x5 128->128 B=2 13x21 virtual, amax prior  | ragged on both axes; out_amax starts above max|out| and must survive
    1x1 256-> 64 B=5  9x17 virtual              | `confusion` width; 1x1 always 2 images: 3 groups, last half empty
    3x3  16->128 B=1  5x3  plain                | ONE channel block (odd: zero-weight padding block / non-DBH 3x3), < one tile
    5x5  48-> 64 B=2  1x1  virtual              | odd block count; image smaller than the 5x5 halo (128 output elements)
    1x1 128->128 B=3 13x21 plain                | tiled 1x1 with 128 output channels
    3x3 128-> 64 B=70 12x12 plain               | 35 x 4 = 140 workgroups (2-image forms): XCD remap with grid % 8 != 0
    5x5  64->128 B=3 40x40 plain                | 5x5 x 128 channels (512-thread fp16x3 form), 25 tiles x 1 group
    3x3 256->128 B=2  9x17 virtual              | 16 channel blocks, even: double-buffered-halo 3x3 of bf16x6
    1x1  64-> 64 B=1 40x40 virtual              | B = 1: second image slot of every workgroup absent

  forward, epi_mode 0 of the train instantiation (FWD0_CASES)
    1x1 256-> 64 B=2 40x40 virtual in, plain res, ReLU        | MSRB `confusion` (bf16: streaming kernel)
    1x1 256-> 64 B=3 13x21 virtual in, VIRTUAL res, ReLU      | first MSRB: `output += x` of a stored pre-BatchNorm x
    3x3  64-> 64 B=5  9x17 plain in, plain res, ReLU          | ResBlock tail; four different offsets
    3x3  64-> 64 B=1  5x3  plain in, no res, ReLU             | ResBlock conv1
    1x1 128->128 B=2  1x1  virtual in, no res, no ReLU        | bf16: the TILED 1x1 (C_out 128); 1x1 image
    5x5  48->128 B=3 13x21 virtual in, virtual res, scale     | odd blocks, `scale` and `shift` both set, no ReLU
    5x5  16-> 64 B=2  9x17 plain in, plain res, no ReLU       | one channel block
    1x1  64-> 64 B=70 12x12 plain in, plain res, ReLU         | large grid
    3x3 128->128 B=2 40x40 virtual in, plain res, ReLU        | 512-thread fp16x3 form with the residual epilogue

  data gradient (DGRAD_CASES; conv K -> C_in, the launch writes N channels from ci0)
    3x3 K= 64 N= 64 ci0=0   B=3 40x40 res, mask + BatchNorm sums
    5x5 K=128 N=128 ci0=64  B=2 13x21 res, scale, mask + sums   | ci0 > 0 inside a 192-channel conv
    1x1 K= 64 N=128 ci0=128 B=5  9x17 mask + sums               | `confusion` dgrad
    3x3 K= 16 N= 64 ci0=0   B=1  5x3  res, mask + sums          | one channel block
    5x5 K= 48 N= 64 ci0=64  B=2  1x1  res, mask, NO bn_a        | no slab is written: its NaN pre-fill survives
    1x1 K=256 N= 64 ci0=0   B=3 13x21 scale, unmasked partial   | epi_mode 0, no mask: first half of a two-conv gradient
    3x3 K=128 N=128 ci0=0   B=70 12x12 res, mask + sums         | large grid
    5x5 K= 64 N= 64 ci0=0   B=3 40x40 res, unmasked partial
    3x3 K=256 N=128 ci0=0   B=2  9x17 res, mask + sums          | four different offsets
    1x1 K=128 N= 64 ci0=64  B=1 40x40 res, mask + sums

Bars (the project's own, see test_gpu_train.py): f32 / bf16x6 / fp16x3 max-norm relative to the reference's max < 1e-5 against
fp64 on the fp32 operands; bf16op the same bar against fp64 on the bf16-ROUNDED operands (a virtual input is rounded after the
fp32 transform, as the kernel does); bf16x3 1e-4 against unrounded operands; bf16 storage: fp64 on the bf16-rounded operands,
output >= 99 % bit-identical to bf16(ref), no element beyond 1.01 bf16 ulp or 3e-6 max|ref|, BatchNorm-backward sums 1e-4,
Welford statistics 1e-5 (they come from the unrounded accumulator).  Where a bf16 tensor has fewer than 100 elements ONE
differing element alone would break 99 %: the share is then not asserted, the ulp bound is (no case above is that small; the
1x1-image cases have 128 / 256 elements).  out_amax is an fp32 scalar of the UNROUNDED values: checked (==) on fp32 tensors only.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from _conv_ex_cases import (NAN, IMPLS, TOL, SUM_TOL, GUARD, FWD1_CASES, FWD0_CASES, DGRAD_CASES,         # noqa: F401
                            q16, fma32, relerr, images_per_workgroup, operands, check_tensor, entry_counts, check_welford_host)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


# ---------------------------------------------------------------------------------------------------------------- plumbing
def cb16(x, ctot, coff, dtype=torch.float32):
    """NCHW (cpu) -> flat CB16 device buffer [B][ctot/16][H*W][16]; channels outside [coff, coff + C) are NaN."""
    B, C, H, W = x.shape
    buf = torch.full((B, ctot // 16, H * W, 16), NAN, dtype=dtype)
    buf[:, coff // 16:(coff + C) // 16] = x.reshape(B, C // 16, 16, H * W).permute(0, 1, 3, 2).to(dtype)
    return buf.reshape(-1).cuda()


def nchw(buf, B, ctot, H, W):
    return buf.cpu().float().view(B, ctot // 16, H * W, 16).permute(0, 1, 3, 2).reshape(B, ctot, H, W)


def act_dtype(ns):
    return torch.bfloat16 if ns == -1 else torch.float32


def dev(t):
    return None if t is None else t.cuda().contiguous()


def pack_fwd(ns, w):
    from tactilesr_amd.model._train import _pack
    wd = dev(w)
    wa = wd.abs().max().reshape(1) if ns == -2 else None
    return _pack(wd, w.shape[0], w.shape[1], w.shape[2], ns, wa), wa


def check_outside_untouched(full, coff, c):
    assert torch.isnan(full[:, :coff]).all() and torch.isnan(full[:, coff + c:]).all(), "wrote outside its channel slice"


def slab_geometry(ns, ks, B, H, W, cout):
    """(entries the library reports, images per workgroup, expected valid-pixel count of every entry)."""
    from tactilesr_amd._lib import load
    img = images_per_workgroup(ns, ks)
    entries, want_cnt = entry_counts(img, B, H, W)
    assert entries == load().tsr_conv2d_slab_entries_ex(B, H, W, cout, ks, ns)
    return entries, img, want_cnt


def check_welford(ns, slab, cnt, ref, ks, tol, check_var=True):
    """epi_mode 1 slabs against the fp64 output `ref`: guard band, counts, per-entry means, Chan-merged mean / variance."""
    B, cout, H, W = ref.shape
    _, img, _ = slab_geometry(ns, ks, B, H, W, cout)
    return check_welford_host(slab.cpu(), cnt.cpu(), ref, img, tol, check_var)


def test_every_train_arithmetic_is_parametrized():
    from tactilesr_amd.model._train import TRAIN_IMPLS
    assert all(IMPLS[k] == v for k, v in TRAIN_IMPLS.items())


# ------------------------------------------------------------------------------------------- 1. forward, epi_mode 1
def _cid(c):
    return "-".join("x" if v is None else str(v) for v in c)


def run_fwd1(T, ns, z, w, s, t, in_coff, out_coff, in_amax=None, prior=None):
    """One epi_mode-1 launch on NaN-filled buffers.  Returns (output over ALL channels of its buffer, slab, counts, amax)."""
    from tactilesr_amd.model._train import conv_ex, Act
    B, cin, H, W = z.shape
    cout, ks = w.shape[0], w.shape[2]
    dt = act_dtype(ns)
    wp, wa = pack_fwd(ns, w)
    zd = cb16(z, cin + 48, in_coff, dt)
    am_in = None
    if ns == -2:
        am_in = torch.tensor([float(z.abs().max()) if in_amax is None else in_amax], device="cuda")
    entries, _, _ = slab_geometry(ns, ks, B, H, W, cout)
    slab = torch.full(((entries + GUARD) * cout * 2,), NAN, device="cuda")
    cnt = torch.full((entries + GUARD,), NAN, device="cuda")
    out = torch.full((B * (cout + 48) * H * W,), NAN, dtype=dt, device="cuda")
    am = None if prior is None or ns == -1 else torch.tensor([prior], device="cuda")
    conv_ex(B=B, H=H, W=W, src=Act(zd, cin + 48, in_coff, cin, dev(s), dev(t), amax=am_in), w=wp, cout=cout, ks=ks, out=out,
            out_ctot=cout + 48, out_coff=out_coff, epi_mode=1, slab=slab, slab_cnt=cnt, nsplit=ns, w_amax=wa, out_amax=am)
    torch.cuda.synchronize()
    return nchw(out, B, cout + 48, H, W), slab, cnt, am


@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("case", FWD1_CASES, ids=_cid)
def test_forward_raw_output_and_welford_slabs(T, case, impl):
    """epi_mode 1: raw output slice + Welford partials per (workgroup, image slot), plain and virtual input."""
    ks, cin, cout, B, H, W, virt, in_coff, out_coff, prior = case
    ns = IMPLS[impl]
    g = torch.Generator().manual_seed(1000 + ks * 7 + cin + cout + B + H)
    z = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
    s = torch.rand(cin, generator=g) + 0.5 if virt else None
    t = torch.randn(cin, generator=g) * 0.3 if virt else None
    zs, a, wr = operands(ns, z, w, s, t)
    full, slab, cnt, am = run_fwd1(T, ns, zs, w, s, t, in_coff, out_coff, prior=prior)
    ref = F.conv2d(a, wr, padding=ks // 2)
    got = full[:, out_coff:out_coff + cout]
    check_outside_untouched(full, out_coff, cout)
    txt = check_tensor(ns, got, ref)
    st = check_welford(ns, slab, cnt, ref, ks, TOL[ns])
    print(f"[conv_ex fwd1] {impl} k{ks} {cin}->{cout} B={B} {H}x{W} virtual={virt}: out {txt}, {st}")
    if am is not None:
        assert am.item() == max(prior, float(got.abs().max()))


# ------------------------------------------------------------------------------------------- 2. forward, epi_mode 0
@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("case", FWD0_CASES, ids=_cid)
def test_forward_affine_residual_relu_epilogue(T, case, impl):
    """epi_mode 0 of the TRAIN instantiation: out = act(conv(a) * scale + shift + residual), the residual plain or
    virtual (relu(r * res_scale + res_shift), fp32, not rounded), the input plain or virtual."""
    from tactilesr_amd.model._train import conv_ex, Act
    ks, cin, cout, B, H, W, virt, res, relu, use_scale, in_coff, out_coff, res_coff = case
    ns = IMPLS[impl]
    dt = act_dtype(ns)
    g = torch.Generator().manual_seed(2000 + ks * 7 + cin + cout + B + H)
    z = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
    s = torch.rand(cin, generator=g) + 0.5 if virt else None
    t = torch.randn(cin, generator=g) * 0.3 if virt else None
    scale = torch.rand(cout, generator=g) + 0.5 if use_scale else None
    shift = torch.randn(cout, generator=g) * 0.1
    r = torch.randn(B, cout, H, W, generator=g)
    rs, rt = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    zs, a, wr = operands(ns, z, w, s, t)
    rq = q16(r) if ns == -1 else r
    ref = F.conv2d(a, wr, padding=ks // 2)
    if use_scale:
        ref = ref * scale.double().view(1, -1, 1, 1)
    ref = ref + shift.double().view(1, -1, 1, 1)
    if res == "virtual":
        ref = ref + F.relu(fma32(rq, rs, rt)).double()
    elif res:
        ref = ref + rq.double()
    ref = F.relu(ref) if relu else ref
    wp, wa = pack_fwd(ns, w)
    zd = cb16(zs, cin + 48, in_coff, dt)
    am_in = torch.tensor([float(zs.abs().max())], device="cuda") if ns == -2 else None
    rA = None
    if res:
        rA = Act(cb16(rq, cout + 48, res_coff, dt), cout + 48, res_coff, cout, *((dev(rs), dev(rt)) if res == "virtual" else ()))
    out = torch.full((B * (cout + 48) * H * W,), NAN, dtype=dt, device="cuda")
    am = None if ns == -1 else torch.zeros(1, device="cuda")
    slab = torch.full((64,), NAN, device="cuda")
    conv_ex(B=B, H=H, W=W, src=Act(zd, cin + 48, in_coff, cin, dev(s), dev(t), amax=am_in), w=wp, cout=cout, ks=ks, out=out,
            out_ctot=cout + 48, out_coff=out_coff, scale=dev(scale), shift=dev(shift), relu=relu, res=rA, nsplit=ns, w_amax=wa,
            out_amax=am, slab=slab, slab_cnt=slab)
    torch.cuda.synchronize()
    full = nchw(out, B, cout + 48, H, W)
    got = full[:, out_coff:out_coff + cout]
    check_outside_untouched(full, out_coff, cout)
    txt = check_tensor(ns, got, ref)
    print(f"[conv_ex fwd0] {impl} k{ks} {cin}->{cout} B={B} {H}x{W} virtual={virt} res={res} relu={relu}: out {txt}")
    assert torch.isnan(slab).all()                       # epi_mode 0 writes no statistics
    if am is not None:
        assert am.item() == float(got.abs().max())


# ------------------------------------------------------------------------------------------- 3. data gradient
@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_cid)
def test_dgrad_mask_and_bn_sums_direct(T, case, impl):
    """out == (conv_transpose(dz, w)[ci0 : ci0 + N] * scale + res) * [fma(z, mask_scale, mask_shift) > 0] and, summed over all
    slab entries, sum(out) and sum(out * xhat) per channel (xhat = z * bn_a + bn_b).  Elements whose fp64 pre-activation is
    within 1e-6 of zero (relative to its max) take the device's own decision; their share is capped at 1e-4."""
    from tactilesr_amd.model._train import conv_ex, Act, _pack_dgrad
    ks, K, cin, NP, ci0, B, H, W, use_res, form, use_scale, dz_coff, out_coff, res_coff, mask_coff = case
    ns = IMPLS[impl]
    dt = act_dtype(ns)
    g = torch.Generator().manual_seed(3000 + ks * 7 + K + cin + B + H)
    dz = torch.randn(B, K, H, W, generator=g)
    w = torch.randn(K, cin, ks, ks, generator=g) * 0.05
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
        x = x * scale.double().view(1, -1, 1, 1)
    if use_res:
        x = x + extra.double()
    wd = dev(w)
    wa = wd.abs().max().reshape(1) if ns == -2 else None
    wp = _pack_dgrad(wd, K, cin, ks, ci0, NP, ns, wa)
    am_in = torch.tensor([float(dz.abs().max())], device="cuda") if ns == -2 else None
    src = Act(cb16(dz, K + 48, dz_coff, dt), K + 48, dz_coff, K, amax=am_in)
    rA = Act(cb16(extra, NP + 48, res_coff, dt), NP + 48, res_coff, NP) if use_res else None
    mk = Act(cb16(z, NP + 48, mask_coff, dt), NP + 48, mask_coff, NP, dev(ms), dev(mh), dev(ba), dev(bb))
    entries, _, _ = slab_geometry(ns, ks, B, H, W, NP)
    slab = torch.full(((entries + GUARD) * NP * 2,), NAN, device="cuda")
    out = torch.full((B * (NP + 48) * H * W,), NAN, dtype=dt, device="cuda")
    am = None if ns == -1 else torch.zeros(1, device="cuda")
    kw = dict(B=B, H=H, W=W, src=src, w=wp, cout=NP, ks=ks, out=out, out_ctot=NP + 48, out_coff=out_coff, scale=dev(scale),
              res=rA, slab=slab, nsplit=ns, w_amax=wa, out_amax=am)
    if form == "partial":
        conv_ex(epi_mode=0, **kw)
    else:
        conv_ex(epi_mode=2, mask=mk, bn=form == "bn", **kw)
    torch.cuda.synchronize()
    full = nchw(out, B, NP + 48, H, W)
    got = full[:, out_coff:out_coff + NP]
    check_outside_untouched(full, out_coff, NP)
    share = 0.0
    if form != "partial":
        pre = z.double() * ms.double().view(1, -1, 1, 1) + mh.double().view(1, -1, 1, 1)
        near = pre.abs() < 1e-6 * pre.abs().max()
        share = float(near.double().mean())
        assert share <= 1e-4
        on = torch.where(near, got != 0, pre > 0)
        x = torch.where(on, x, torch.zeros_like(x))
    txt = check_tensor(ns, got, x)
    sl = slab.cpu().double().view(entries + GUARD, NP, 2)
    st = "no slab"
    if form == "bn":
        assert torch.isnan(sl[entries:]).all(), "an entry was written out of range"
        assert torch.isfinite(sl[:entries]).all(), "an entry was not written"
        xhat = z.double() * ba.double().view(1, -1, 1, 1) + bb.double().view(1, -1, 1, 1)
        s1, s2 = x.sum(dim=(0, 2, 3)), (x * xhat).sum(dim=(0, 2, 3))
        sums = sl[:entries].sum(0)
        e1, e2 = relerr(sums[:, 0], s1), relerr(sums[:, 1], s2)
        st = f"sums {e1:.1e} / {e2:.1e}"
        assert e1 < SUM_TOL[ns] and e2 < SUM_TOL[ns], st
    else:
        assert torch.isnan(sl).all(), "a launch without bn_a wrote the slab"
    print(f"[conv_ex dgrad] {impl} k{ks} {K}->{cin}[{ci0}:{ci0 + NP}] B={B} {H}x{W} {form} res={use_res}: out {txt}, {st}, "
          f"near-zero mask share {share:.1e}")
    if am is not None:
        assert am.item() == float(got.abs().max())


@pytest.mark.parametrize("impl", ["bf16x6", "fp16x3"])
@pytest.mark.parametrize("ks,cin,cout,B,H,W,NP", [(3, 64, 64, 3, 40, 40, 64), (5, 128, 128, 2, 16, 24, 64),
                                                  (1, 256, 64, 2, 40, 40, 64), (3, 448, 64, 1, 40, 40, 64),
                                                  (1, 256, 64, 1, 40, 40, 128), (1, 256, 64, 3, 40, 40, 128),
                                                  (5, 128, 128, 5, 16, 24, 128), (3, 128, 128, 1, 40, 40, 128)])
def test_dgrad_bn_backward_end_to_end_vs_autograd(T, ks, cin, cout, B, H, W, NP, impl):
    """test_conv2d_dgrad_with_mask_and_bn_sums of test_gpu_train.py (nsplit = 0) in the other fp32-equivalent arithmetics: the
    dgrad launch + tsr_bn_bwd_finalize + tsr_bn_bwd_apply against autograd through relu(batch_norm(z)) -> conv, same cases,
    same 1e-5 bars."""
    from tactilesr_amd.model._train import conv_ex, Act, _pack_dgrad
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_double as D
    ns = IMPLS[impl]
    g = torch.Generator().manual_seed(ks + cin)
    z = torch.randn(B, cin, H, W, generator=g)
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
    dy = torch.randn(B, cout, H, W, generator=g)
    extra = torch.randn(B, cin, H, W, generator=g) * 0.1
    zr = z.clone().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = F.relu(F.batch_norm(zr, None, None, gm, bt, True, 0.1, 1e-5))
    y = F.conv2d(a, w, padding=ks // 2)
    loss = (y * dy).sum() + (a * extra).sum()
    gz, ggm, gbt = torch.autograd.grad(loss, (zr, gm, bt))
    mean = z.mean(dim=(0, 2, 3))
    var = z.var(dim=(0, 2, 3), unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    vec = torch.stack([gamma * invstd, beta - mean * gamma * invstd, invstd, -mean * invstd]).cuda()
    zd, dyd, exd = T.to_cb16(z.cuda()), T.to_cb16(dy.cuda()), T.to_cb16(extra.cuda())
    gbuf = torch.empty(B * cin * H * W, device="cuda")
    lib = load()
    entries = lib.tsr_conv2d_slab_entries_ex(B, H, W, NP, ks, ns)
    work = torch.empty(512 * 128 * 3, dtype=torch.float64, device="cuda")
    wd = w.cuda().contiguous()
    wa = wd.abs().max().reshape(1) if ns == -2 else None
    am_in = dy.abs().max().reshape(1).cuda() if ns == -2 else None
    dgam, dbet = [], []
    for o in range(0, cin, NP):
        slab = torch.empty(entries * NP * 2, device="cuda")
        wp = _pack_dgrad(wd, cout, cin, ks, o, NP, ns, wa)
        mk = Act(zd, cin, o, NP, vec[0, o:o + NP], vec[1, o:o + NP], vec[2, o:o + NP], vec[3, o:o + NP])
        conv_ex(B=B, H=H, W=W, src=Act(dyd, cout, 0, cout, amax=am_in), w=wp, cout=NP, ks=ks, out=gbuf, out_ctot=cin,
                out_coff=o, res=Act(exd, cin, o, NP), epi_mode=2, mask=mk, bn=True, slab=slab, nsplit=ns, w_amax=wa)
        out = torch.empty(5, NP, device="cuda")
        call("tsr_bn_bwd_finalize", ptr(slab), I(entries), I(NP), D(float(B * H * W)), ptr(vec[0, o:o + NP]),
             ptr(vec[2, o:o + NP]), ptr(vec[3, o:o + NP]), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
             ptr(out[4]), ptr(work), stream())
        am = torch.zeros(1, device="cuda")
        call("tsr_bn_bwd_apply", ptr(gbuf), I(cin), I(o), ptr(zd), I(cin), I(o), ptr(out[2]), ptr(out[3]), ptr(out[4]),
             I(NP), I(B), I(H * W), ptr(am), stream())
        assert am.item() == T.from_cb16(gbuf, B, cin, H, W)[:, o:o + NP].abs().max().item()
        dgam.append(out[0].clone())
        dbet.append(out[1].clone())
    e = relerr(T.from_cb16(gbuf, B, cin, H, W).cpu(), gz), relerr(torch.cat(dgam).cpu(), ggm), relerr(torch.cat(dbet).cpu(), gbt)
    print(f"[conv_ex dgrad e2e] {impl} k{ks} {cout}->{cin} N={NP} B={B} {H}x{W}: gz {e[0]:.1e}, dgamma {e[1]:.1e}, dbeta {e[2]:.1e}")
    assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 1e-5


# ------------------------------------------------------------------- 4. virtual input under fp16x3: the in-kernel bound
S4_SHAPES = [(3, 128, 128), (5, 64, 64), (1, 256, 64)]
S4_B, S4_H, S4_W = 2, 13, 21


def s4_inputs(ks, cin, cout, variant):
    g = torch.Generator().manual_seed(4000 + ks + cin)
    z = torch.randn(S4_B, cin, S4_H, S4_W, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * 0.05
    s = torch.rand(cin, generator=g) + 0.5
    t = torch.randn(cin, generator=g) * 0.3
    if variant == "t_dominates":                # z tiny, t_c = 3: the bound is its `+ max|t_c|` term alone
        z = z * 1e-3
        t = torch.full((cin,), 3.0)
    elif variant != "plain":
        s[5] = 300.0                            # a near-constant channel: invstd up to 1 / sqrt(eps) = 316
        z[:, 5] /= 300.0
    if variant == "s300_out41":
        z[0, 1, 2, 3] = 41.0
    if variant == "s300_out1e3":
        z[0, 1, 2, 3] = 1.0e3
    return z, w, s, t


def f16x3_model(a, w, bound, ks):
    """fp64 model of the documented scheme (include/tactilesr_hip.h, csrc/conv_mfma_split16.hip): a * sx = h1 + h2 and
    w * sw = g1 + g2 in fp16 with the power-of-two scales that put `bound` and max|w| into [2^13, 2^14), the three products
    h1 g1 + h1 g2 + h2 g1, the scales undone exactly.  Never reads anything the kernel wrote."""
    sx = 2.0 ** (13 - math.floor(math.log2(bound)))
    sw = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    xs, ws = a.float() * sx, w.float() * sw
    h1, g1 = xs.half().float(), ws.half().float()
    h2, g2 = (xs - h1).half().float(), (ws - g1).half().float()
    c = lambda u, v: F.conv2d(u.double(), v.double(), padding=ks // 2)
    return (c(h1, g1) + c(h1, g2) + c(h2, g1)) / (sx * sw)


@pytest.mark.parametrize("variant", ["plain", "s300", "s300_out41", "s300_out1e3", "stale_amax", "t_dominates"])
@pytest.mark.parametrize("ks,cin,cout", S4_SHAPES)
def test_fp16x3_virtual_input_bound(T, ks, cin, cout, variant):
    """fp16x3 forward with a virtual input: the kernels bound max|a| by in_amax * max|s_c| + max|t_c| and derive the operand
    scale from that.  One BatchNorm scale of 300 inflates the bound for every channel (by a few hundred: the fp64 model of
    the scheme stays <= 2.6e-7, so the bar stays 1e-5); a stale in_amax (2^10 too large: legal, it is an upper bound) pushes
    the low plane towards fp16's subnormals -- the model of exactly that case is computed here and decides its bar: 1e-5 if
    the model stays under 5e-6, twice the model otherwise; `t_dominates` is the case an understated bound would overflow
    (its output is constant per channel to 1e-3, so its variance -- 1e-7 of mean^2 -- is a difference of nearly equal
    numbers in ANY fp32 convolution: there the bar holds for the output, the entry means and the merged mean, and the
    variance is printed only)."""
    ns = -2
    z, w, s, t = s4_inputs(ks, cin, cout, variant)
    amax = float(z.abs().max()) * (1024.0 if variant == "stale_amax" else 1.0)
    _, a, wr = operands(ns, z, w, s, t)
    full, slab, cnt, _ = run_fwd1(T, ns, z, w, s, t, 16, 32, in_amax=amax)
    ref = F.conv2d(a, wr, padding=ks // 2)
    got = full[:, 32:32 + cout]
    check_outside_untouched(full, 32, cout)
    bound = float(torch.tensor(amax, dtype=torch.float32) * s.abs().max() + t.abs().max())
    model = relerr(f16x3_model(a, w, bound, ks), ref)
    bar = 1e-5 if (variant != "stale_amax" or model < 5e-6) else 2 * model
    assert torch.isfinite(got).all()
    e = relerr(got, ref)
    st = check_welford(ns, slab, cnt, ref, ks, bar, check_var=variant != "t_dominates")
    print(f"[conv_ex fp16x3 bound] k{ks} {cin}->{cout} {variant}: bound / max|a| {bound / float(a.abs().max()):.1f}, "
          f"fp64 model of the scheme {model:.1e}, kernel {e:.1e} (bar {bar:.1e}), {st}")
    assert e < bar


@pytest.mark.parametrize("bad", [NAN, float("inf")])
@pytest.mark.parametrize("ks,cin,cout", S4_SHAPES)
def test_fp16x3_virtual_input_non_finite_stays_in_its_receptive_field(T, ks, cin, cout, bad):
    """A NaN / Inf raw element of a VIRTUAL input reaches exactly the outputs whose window covers it and the Welford entries
    of the (tile, image) pairs those outputs lie in; everything else is bit-identical to the clean run (in_amax is the clean
    tensor's: the producers' atomic max skips non-finite values).  (0, 0, 0, 0) is also the dummy element padding slots read."""
    ns, P = -2, ks // 2
    B, H, W = S4_B, S4_H, S4_W
    z, w, s, t = s4_inputs(ks, cin, cout, "plain")
    amax = float(z.abs().max())
    clean, cslab, ccnt, _ = run_fwd1(T, ns, z, w, s, t, 16, 32, in_amax=amax)
    entries, img, _ = slab_geometry(ns, ks, B, H, W, cout)
    tx_n, tiles = (W + 7) // 8, ((H + 7) // 8) * ((W + 7) // 8)
    for (b, c, y, x) in [(0, 0, 0, 0), (1, cin - 1, 7, 9)]:
        zb = z.clone()
        zb[b, c, y, x] = bad
        got, slab, cnt, _ = run_fwd1(T, ns, zb, w, s, t, 16, 32, in_amax=amax)
        win = torch.zeros(B, 1, H, W, dtype=torch.bool)
        win[b, 0, max(0, y - P):y + P + 1, max(0, x - P):x + P + 1] = True
        winc = win.expand(B, cout, H, W)
        g, cl = got[:, 32:32 + cout], clean[:, 32:32 + cout]
        assert not torch.isfinite(g[winc]).any(), "every output whose window covers the bad element is non-finite"
        assert torch.equal(g[~winc], cl[~winc]), "no other output changes"
        check_outside_untouched(got, 32, cout)
        sl, csl = slab.cpu().view(entries + GUARD, cout, 2), cslab.cpu().view(entries + GUARD, cout, 2)
        assert torch.equal(cnt.cpu()[:entries], ccnt.cpu()[:entries])
        for e in range(entries):
            eb, tl = (e // (tiles * img)) * img + e % img, (e // img) % tiles
            y0, x0 = (tl // tx_n) * 8, (tl % tx_n) * 8
            if eb < B and bool(win[eb, 0, y0:y0 + 8, x0:x0 + 8].any()):
                assert not torch.isfinite(sl[e]).any(), f"entry {e} holds outputs of the bad element's window"
            else:
                assert torch.equal(sl[e], csl[e]), f"entry {e} must not change"


# ------------------------------------------------------------------------------------------- 5. packers
def _weights_with_max(kind, shape, g):
    w = torch.randn(*shape, generator=g) * 0.05
    if kind == "zero":
        return torch.zeros(*shape)
    w = w.clamp(-0.2, 0.2)
    w.view(-1)[7] = {"pow2": -0.25, "below_one": 1.0 - 2.0 ** -24, "plain": 0.2345}[kind]
    return w


@pytest.mark.parametrize("kind", ["pow2", "below_one", "zero", "plain"])
@pytest.mark.parametrize("cout,cin,ks", [(64, 64, 3), (128, 48, 5), (64, 256, 1), (128, 128, 5)])
def test_f16s_pack_host_scale_equals_device_scale(T, cout, cin, ks, kind):
    """tsr_pack_conv_weight_f16s (host wscale = 2^(13 - floor(log2 max|w|))) and tsr_pack_conv_weight_f16s_dev (w_amax on the
    device; scale 1 for an all-zero weight) produce bit-identical buffers."""
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_float as Fl
    g = torch.Generator().manual_seed(cout + cin + ks)
    w = _weights_with_max(kind, (cout, cin, ks, ks), g).cuda().contiguous()
    mx = float(w.abs().max())
    wscale = 2.0 ** (13 - math.floor(math.log2(mx))) if mx > 0 else 1.0
    n = load().tsr_conv_weight_bf16s_elems(cout, cin, ks, 2)
    a = torch.full((n,), 0x7A7A, dtype=torch.int16, device="cuda")
    b = a.clone()
    call("tsr_pack_conv_weight_f16s", ptr(w), ptr(a), I(cout), I(cin), I(ks), Fl(wscale), stream())
    call("tsr_pack_conv_weight_f16s_dev", ptr(w), ptr(b), I(cout), I(cin), I(ks), ptr(w.abs().max().reshape(1)), stream())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert not torch.equal(a, torch.full_like(a, 0x7A7A))           # (both were written)


@pytest.mark.parametrize("kind", ["pow2", "below_one", "zero", "plain"])
@pytest.mark.parametrize("K,cin,ks,ci0,NP", [(128, 192, 3, 64, 128), (48, 64, 5, 0, 64), (64, 256, 1, 128, 128)])
def test_f16s_dgrad_pack_host_scale_equals_device_scale(T, K, cin, ks, ci0, NP, kind):
    """The same for the data-gradient packers: tsr_pack_conv_weight_dgrad_f16s (no caller in the package) vs ..._dgrad_f16s_dev."""
    from tactilesr_amd._lib import call, ptr, stream, load, c_int as I, c_float as Fl
    g = torch.Generator().manual_seed(K + cin + ks)
    w = _weights_with_max(kind, (K, cin, ks, ks), g).cuda().contiguous()
    mx = float(w.abs().max())
    wscale = 2.0 ** (13 - math.floor(math.log2(mx))) if mx > 0 else 1.0
    n = load().tsr_conv_weight_bf16s_elems(NP, K, ks, 2)
    a = torch.full((n,), 0x7A7A, dtype=torch.int16, device="cuda")
    b = a.clone()
    call("tsr_pack_conv_weight_dgrad_f16s", ptr(w), ptr(a), I(K), I(cin), I(ks), I(ci0), I(NP), Fl(wscale), stream())
    call("tsr_pack_conv_weight_dgrad_f16s_dev", ptr(w), ptr(b), I(K), I(cin), I(ks), I(ci0), I(NP),
         ptr(w.abs().max().reshape(1)), stream())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
