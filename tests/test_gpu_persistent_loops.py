"""Kernel-level tests of the PERSISTENT-WORKGROUP LOOPS: the four kernel families that cap their grid and let a workgroup walk
a range of work items, at batch sizes where a workgroup really handles several items, on data in which consecutive items
differ by a factor -- against fp64, element by element and slab entry by slab entry.

    1. fwd1x1_b16k_kernel        (tsr_conv2d_ex, nsplit -3, ks 1, epi_mode 0)   4-slot LDS ring, 3 items requested ahead, the
                                                                               store of step s issued in step s + 1
    2. dgrad1x1_b16k_kernel<4>   (nsplit -3, ks 1, epi_mode 2)                  4 pixel groups in flight, sums carried over a
                                                                               range, ONE slab entry per workgroup
    3. conv1x1_b16_ex_kernel<64> (nsplit -1, ks 1, C_out 64, epi_mode 0)        grid-stride loop over (image group, tile)
    4. tPSFNet forward / backward                                              `for (b = blockIdx.x; b < B; b += gridDim.x)`

The other kernel-level tests of these launches (test_gpu_train.py, test_gpu_conv_ex.py, test_gpu_tpsf.py) stay below the grid
caps, or compare later iterations with copies of the same data.  Case tables, launcher arithmetic and references live in
tests/_persistent_loops.py; tests/test_persistent_loops_cpu.py checks there that every row reaches the loop state it is here for.

Every operand lives in a buffer 48 channels wider than its slice, at a non-zero channel offset, NaN outside the slice; every
output buffer is NaN-filled and must still be NaN outside the output slice.  Bars: the project's own for bf16 storage
(check_tensor(-1, ...) of test_gpu_conv_ex.py: >= 99 % of the outputs identical to bf16(ref), none beyond 1.01 bf16 ulp or
3e-6 max|ref|), 1e-4 of the largest reference entry for each slab entry's BatchNorm-backward sums, 1e-5 for tPSFNet.
"""
import pytest
import torch

from oracle import tactilesr_oracle as O
from test_gpu_conv_ex import NAN, GUARD, SUM_TOL, cb16, nchw, dev, check_tensor, check_outside_untouched, pack_fwd, relerr
import _persistent_loops as P

pytestmark = pytest.mark.gpu

WIDER = 48


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


def run_forward(ns, c, d, wp):
    """One epi_mode-0 1x1 launch (bias, residual, ReLU) on NaN-filled bf16 buffers; returns the output over ALL channels."""
    from tactilesr_amd.model._train import conv_ex, Act
    dt = torch.bfloat16
    src = Act(cb16(d["z"], c.cin + WIDER, c.in_coff, dt), c.cin + WIDER, c.in_coff, c.cin, dev(d["s"]), dev(d["t"]))
    rA = None
    if c.res:
        virt = (dev(d["rs"]), dev(d["rt"])) if c.res == "virtual" else ()
        rA = Act(cb16(d["r"], P.COUT + WIDER, c.res_coff, dt), P.COUT + WIDER, c.res_coff, P.COUT, *virt)
    out = torch.full((c.B * (P.COUT + WIDER) * c.H * c.W,), NAN, dtype=dt, device="cuda")
    slab = torch.full((64,), NAN, device="cuda")
    conv_ex(B=c.B, H=c.H, W=c.W, src=src, w=wp, cout=P.COUT, ks=1, out=out, out_ctot=P.COUT + WIDER, out_coff=c.out_coff,
            shift=dev(d["bias"]), relu=c.relu, res=rA, nsplit=ns, slab=slab, slab_cnt=slab)
    torch.cuda.synchronize()
    assert torch.isnan(slab).all()                       # epi_mode 0 writes no statistics
    return nchw(out, c.B, P.COUT + WIDER, c.H, c.W)


# ------------------------------------------------------------------------------------------- 1. fwd1x1_b16k: the ring
@pytest.mark.parametrize("c", P.FWD1X1_CASES, ids=P.case_id)
def test_fwd1x1_b16k_ring_over_several_items(T, c):
    """`per` = 2 .. 9 items per workgroup: fewer than, as many as and more than the ring's slots; ranges that begin inside an
    image and cross image boundaries; ragged items; workgroups with an empty range; the deferred store of a range's last item."""
    from tactilesr_amd._lib import load, call, ptr, stream, c_int as I
    lib = load()
    assert lib.tsr_conv2d_ex_fwd1x1_b16k(P.COUT, c.cin) == 1
    d = P.fwd_inputs(c)
    wp = torch.empty(lib.tsr_conv_weight_b16k_elems(P.COUT, c.cin, 1), dtype=torch.bfloat16, device="cuda")
    call("tsr_pack_conv_weight_b16k", ptr(dev(d["w"])), ptr(wp), I(P.COUT), I(c.cin), I(1), stream())
    full = run_forward(-3, c, d, wp)
    check_outside_untouched(full, c.out_coff, P.COUT)
    txt = check_tensor(-1, full[:, c.out_coff:c.out_coff + P.COUT], d["ref"])
    print(f"[loops fwd1x1_b16k] {c.cin}->64 B={c.B} {c.H}x{c.W} items {c.total} per {c.per} res={c.res} relu={c.relu}: {txt}")


# ------------------------------------------------------------------------- 2. dgrad1x1_b16k: carried sums, one entry per workgroup
@pytest.mark.parametrize("c", P.DGRAD1X1_CASES, ids=P.case_id)
def test_dgrad1x1_b16k_carried_sums_one_entry_per_workgroup(T, c):
    """Output against bf16(mask * conv_transpose(dz, bf16(w))); EVERY slab entry against the fp64 sums over exactly its range of
    pixel groups; entries of workgroups with an empty range exactly 0; the guard band behind the last entry still NaN.  One
    case runs once more without bn_a: the same output bit for bit, and its NaN-filled slab untouched."""
    from tactilesr_amd.model._train import conv_ex, Act, _pack_dgrad
    from tactilesr_amd._lib import load
    lib = load()
    B, H, W, N = c.B, c.H, c.W, P.DG_N
    assert lib.tsr_conv2d_ex_dgrad_b16k(N, P.DG_K, 1) == 1
    entries = lib.tsr_conv2d_slab_entries_ex(B, H, W, N, 1, -3)
    assert entries == P.DGRAD1X1_CAP == 2048
    d = P.dgrad_inputs(c)
    dt = torch.bfloat16
    wp = _pack_dgrad(dev(d["w"]), P.DG_K, P.DG_CIN, 1, c.ci0, N, -3)
    src = Act(cb16(d["dz"], P.DG_K + WIDER, c.dz_coff, dt), P.DG_K + WIDER, c.dz_coff, P.DG_K)
    mk = Act(cb16(d["z"], N + WIDER, c.mask_coff, dt), N + WIDER, c.mask_coff, N, dev(d["ms"]), dev(d["mh"]), dev(d["ba"]),
             dev(d["bb"]))

    def launch(bn):
        slab = torch.full(((entries + GUARD) * N * 2,), NAN, device="cuda")
        out = torch.full((B * (N + WIDER) * H * W,), NAN, dtype=dt, device="cuda")
        conv_ex(B=B, H=H, W=W, src=src, w=wp, cout=N, ks=1, out=out, out_ctot=N + WIDER, out_coff=c.out_coff, epi_mode=2,
                mask=mk, bn=bn, slab=slab, nsplit=-3)
        torch.cuda.synchronize()
        return nchw(out, B, N + WIDER, H, W), slab.cpu().double().view(entries + GUARD, N, 2)

    full, sl = launch(True)
    check_outside_untouched(full, c.out_coff, N)
    txt = check_tensor(-1, full[:, c.out_coff:c.out_coff + N], d["v"])
    grid, per = P.split(c.total, P.DGRAD1X1_CAP)
    used = -(-c.total // per)                                    # workgroups with a non-empty range
    assert torch.isnan(sl[entries:]).all(), "an entry was written out of range"
    assert torch.isfinite(sl[:entries]).all(), "an entry was not written"
    assert bool((sl[used:entries] == 0).all()), "the entry of a workgroup with an empty range is not 0"
    r1, r2 = P.entry_sums(d["v"], grid, per), P.entry_sums(d["v"] * d["xhat"], grid, per)
    e1 = float((sl[:entries, :, 0] - r1).abs().max() / r1.abs().max())
    e2 = float((sl[:entries, :, 1] - r2).abs().max() / r2.abs().max())
    print(f"[loops dgrad1x1_b16k] 64->256[{c.ci0}:{c.ci0 + N}] B={B} {H}x{W} groups {c.total} per {per} "
          f"empty workgroups {entries - used}: out {txt}, worst entry sum v {e1:.1e}, sum v*xhat {e2:.1e}")
    assert e1 < SUM_TOL[-1] and e2 < SUM_TOL[-1], (e1, e2)
    if c.also_without_bn:
        full2, sl2 = launch(False)
        assert torch.equal(full2[:, c.out_coff:c.out_coff + N], full[:, c.out_coff:c.out_coff + N])
        check_outside_untouched(full2, c.out_coff, N)
        assert torch.isnan(sl2).all(), "a launch without bn_a wrote the slab"


# ------------------------------------------------------------------------------------------- 3. conv1x1_b16_ex: grid stride
@pytest.mark.parametrize("c", P.STREAM1X1_CASES, ids=P.case_id)
def test_conv1x1_b16_ex_second_round_of_the_grid_stride_loop(T, c):
    """513 / 516 (image group, tile) items on 512 workgroups: the first workgroups come round a second time, with images whose
    data differ by a factor from those of their first item; B % 4 != 0 leaves image slots of the last group absent."""
    virtual = c.res is not None          # virtual input + plain residual, or plain input and no residual
    d = P.fwd_inputs(c, virtual=virtual)
    wp, _ = pack_fwd(-1, d["w"])
    full = run_forward(-1, c, d, wp)
    check_outside_untouched(full, c.out_coff, P.COUT)
    txt = check_tensor(-1, full[:, c.out_coff:c.out_coff + P.COUT], d["ref"])
    print(f"[loops conv1x1_b16_ex] 256->64 B={c.B} {c.H}x{c.W} items {c.total} virtual={virtual} res={c.res}: {txt}")


# ------------------------------------------------------------------------------------------- 4. tPSFNet: later iterations
def test_tpsf_later_iterations_of_the_persistent_workgroups_vs_fp64():
    """B = 2100 different samples: the forward's 512 workgroups handle up to 5 samples each, tpsf_bwd_dhb's 256 up to 9,
    tpsf_bwd_pool's 2048 up to 2, and the sample before each of them in its workgroup's sequence has a depth 10^2 or 10^3 times
    larger or smaller.  HR, psf, LR_deg and d(alpha, beta, gamma) against the fp64 oracle on 24 indices that include first,
    second and later iterations of every grid, a plateau, a signed and an all-zero depth; bars 1e-5 as in
    test_tpsf_kernels_wide_dynamic_range_batch: HR and psf per sample, LR_deg and the gradient jointly over the compared
    samples -- here jointly over those of one depth scale (b % 5), so that a sample scaled by 10^-2 is not hidden behind one
    scaled by 10^2; within a class the magnitudes are as comparable as they are in that test."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    B = P.TPSF_B
    depth, ab, dl = P.tpsf_inputs()
    idx = torch.tensor(P.TPSF_INDICES)
    # no compared pixel sits where fp32 and fp64 could disagree on `depth > depth.max() - 1e-3`: the fp32 threshold is off by
    # at most half an ulp of the maximum (6e-8 max|depth|); every pixel keeps three times that distance
    sub = depth[idx].double()
    mx = sub.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-3)
    assert float(((sub - (sub.amax(dim=(1, 2), keepdim=True) - 1e-3)).abs() / mx).min()) > 2e-7
    d, a_, dl_ = depth.cuda(), ab.cuda(), dl.cuda()
    HR = torch.full((B, 1, 100, 100), NAN, device="cuda")
    LRd = torch.full((B, 16), NAN, device="cuda")
    psf = torch.full((B, 1, 99, 99), NAN, device="cuda")
    dab = torch.full((B, 3), NAN, device="cuda")
    call("tpsf_forward", ptr(d), ptr(a_), ptr(HR), ptr(LRd), ptr(psf), I(B), stream())
    work = torch.empty(B * 10000, device="cuda")
    call("tpsf_backward", ptr(d), ptr(a_), ptr(HR), ptr(dl_), ptr(dab), ptr(work), I(B), stream())
    torch.cuda.synchronize()
    for t in (HR, LRd, psf, dab):
        assert torch.isfinite(t).all()
    n = len(P.TPSF_INDICES)
    ab64 = ab[idx].double().requires_grad_(True)
    HR64, LR64, psf64 = O.tpsf_forward_from_ab(ab64, depth[idx].double())
    (LR64.reshape(n, 16) * dl[idx].double()).sum().backward()
    HRc, psfc, LRc, dabc = HR.cpu()[idx], psf.cpu()[idx], LRd.cpu()[idx], dab.cpu()[idx]
    e_hr = max(relerr(HRc[i], HR64[i].detach()) for i in range(n))
    e_psf = max(relerr(psfc[i], psf64[i].detach()) for i in range(n))
    e_lr, e_dab = 0.0, 0.0
    for k in range(5):
        cls = idx % 5 == k
        assert int(cls.sum()) >= 4
        e_lr = max(e_lr, relerr(LRc[cls], LR64.detach().reshape(n, 16)[cls]))
        e_dab = max(e_dab, relerr(dabc[cls], ab64.grad[cls]))
    print(f"[loops tpsf] B={B}, 24 samples vs fp64: HR {e_hr:.1e}, psf {e_psf:.1e}, LR_deg {e_lr:.1e}, d(alpha, beta, gamma) {e_dab:.1e}")
    assert e_hr < 1e-5 and e_psf < 1e-5 and e_lr < 1e-5 and e_dab < 1e-5, (e_hr, e_psf, e_lr, e_dab)
