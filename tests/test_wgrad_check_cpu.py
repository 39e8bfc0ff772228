"""Self-test of the weight-gradient comparator (tests/_wgrad_check.py) on the CPU: it must pass torch's own fp32 result and
reject an error of 1e-4 of ONE slice's maximum -- in one tap of one 64 x 64 channel block, and the same error coming from
the image's last (ragged) patch column only."""
import pytest
import torch
import torch.nn.functional as F

import _wgrad_check as WC

KS, CIN, COUT, B, H, W = 3, 128, 128, 2, 13, 21      # case 3 of test_gpu_wgrad.py: four 64 x 64 blocks, ragged on both axes


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(B, CIN, H, W, generator=g)
    dz = torch.randn(B, COUT, H, W, generator=g)
    sc, sh = torch.rand(CIN, generator=g) + 0.5, torch.randn(CIN, generator=g) * 0.3
    a = F.relu(WC.fma32(z, sc, sh))
    return a, dz, WC.reference(a, dz, KS)


def test_fp32_torch_result_passes(case):
    a, dz, ref = case
    got = WC.conv_wgrad(a, dz, KS)
    e, r, _ = WC.check_dw(got, ref, "fp32 torch")
    assert float(ref["e_ref"].max()) < 1e-5        # fp32 summation alone stays far inside the floor of the slice bar here
    assert r <= 1.0 / WC.SLICE_FACTOR + 1e-12      # its own error is e_ref: a quarter of the bar at most
    WC.check_db(dz.sum(dim=(0, 2, 3)), dz.double().sum(dim=(0, 2, 3)), "fp32 torch")


def test_slice_errors_are_per_block_and_tap(case):
    _, _, ref = case
    got = ref["dw"].clone()
    got[70, 5, 2, 0] += 1.0
    rel = WC.slice_errors(got, ref["dw"])
    assert rel.shape == (COUT // 64, CIN // 64, KS, KS)
    assert int((rel > 0).sum()) == 1 and rel[1, 0, 2, 0] > 0


@pytest.mark.parametrize("block,tap", [((1, 0), (0, 2)), ((0, 1), (1, 1))])
def test_rejects_1e4_of_a_slice_maximum_in_one_tap_of_one_block(case, block, tap):
    _, _, ref = case
    cb, ib = block
    sl = (slice(64 * cb, 64 * cb + 64), slice(64 * ib, 64 * ib + 64), tap[0], tap[1])
    got = ref["dw"].clone()
    got[sl][17, 40] += 1e-4 * ref["dw"][sl].abs().max()          # ONE element of the slice
    with pytest.raises(AssertionError, match=f"co block {cb}, ci block {ib}, tap {tap[0]},{tap[1]}"):
        WC.check_dw(got.float(), ref, "perturbed")
    got = ref["dw"].clone()
    got[sl] += 1e-4 * ref["dw"][sl].abs().max()                  # the whole slice
    with pytest.raises(AssertionError, match=f"co block {cb}, ci block {ib}, tap {tap[0]},{tap[1]}"):
        WC.check_dw(got.float(), ref, "perturbed")


def test_rejects_an_error_from_the_last_patch_column_only(case):
    """The error a kernel would make if it mishandled the ragged right patch column (image columns 16 .. 20 of 21): the part
    of dW those output pixels contribute, scaled to 1e-4 of the slice's maximum, in one tap of one block."""
    a, dz, ref = case
    edge = torch.zeros_like(dz)
    edge[..., 8 * ((W - 1) // 8):] = dz[..., 8 * ((W - 1) // 8):]
    part = WC.conv_wgrad(a.double(), edge.double(), KS)
    sl = (slice(64, 128), slice(0, 64), 2, 1)
    got = ref["dw"].clone()
    got[sl] += part[sl] / part[sl].abs().max() * 1e-4 * ref["dw"][sl].abs().max()
    with pytest.raises(AssertionError, match="co block 1, ci block 0, tap 2,1"):
        WC.check_dw(got.float(), ref, "edge")


def test_zero_reference_slices_must_be_exactly_zero():
    """1x1 image, 3x3 kernel: only the centre tap meets an in-image pixel pair; any value in another tap is an error."""
    g = torch.Generator().manual_seed(8)
    a, dz = torch.randn(2, 64, 1, 1, generator=g), torch.randn(2, 64, 1, 1, generator=g)
    ref = WC.reference(a, dz, 3)
    assert int((ref["dw"].abs().amax(dim=(0, 1)) > 0).sum()) == 1
    WC.check_dw(ref["dw"].float(), ref, "1x1 image")
    got = ref["dw"].float().clone()
    got[3, 9, 0, 0] = 1e-30
    with pytest.raises(AssertionError, match="tap 0,0"):
        WC.check_dw(got, ref, "1x1 image")


def test_rejects_non_finite_and_bias_errors(case):
    _, dz, ref = case
    got = ref["dw"].float().clone()
    got[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        WC.check_dw(got, ref, "nan")
    db = dz.double().sum(dim=(0, 2, 3))
    bad = db.clone()
    bad[5] += 1e-4 * db.abs().max()
    with pytest.raises(AssertionError):
        WC.check_db(bad.float(), db, "db")
