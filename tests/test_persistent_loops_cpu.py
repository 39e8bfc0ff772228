"""The case set of tests/test_gpu_persistent_loops.py reaches what it claims: total, grid and items per workgroup of every row,
recomputed with the launchers' arithmetic (constants quoted in tests/_persistent_loops.py), and the loop states they put the
kernels in.  Also a self-test of the bf16 output bar on one wrong 32-pixel item of the largest forward case.  No device is
touched."""
import pytest
import torch

import _persistent_loops as P
from test_gpu_conv_ex import check_tensor, q16


def _ranges(total, cap):
    grid, per = P.split(total, cap)
    return grid, per, [(e * per, min((e + 1) * per, total)) for e in range(grid)]


def test_fwd1x1_cases_reach_every_state_of_the_ring():
    pers, short_last, empties, crossing = set(), 0, 0, 0
    for c in P.FWD1X1_CASES:
        hw = c.H * c.W
        ipi = -(-hw // P.FWD1X1_ITEM_PX)
        grid, per, rng = _ranges(c.B * ipi, P.FWD1X1_CAP)
        assert (c.B * ipi, per) == (c.total, c.per) and grid == P.FWD1X1_CAP, c
        assert (c.in_coff, c.out_coff) != (0, 0) and c.in_coff % 16 == 0 and c.out_coff % 16 == 0
        pers.add(per)
        nonempty = [(a, b) for a, b in rng if b > a]
        empties += grid - len(nonempty)
        short_last += nonempty[-1][1] - nonempty[-1][0] < per
        # ranges cross image boundaries (all but the per = items-per-image row) and, two items per image, begin inside one
        crossing += any(a // ipi != (b - 1) // ipi for a, b in nonempty)
        if ipi == 2 and per % 2:
            assert any(a % ipi for a, _ in nonempty), c
    assert pers == {2, 3, 4, 5, 6, 9}
    assert min(pers) < P.FWD1X1_LOOKAHEAD and {P.FWD1X1_LOOKAHEAD, P.FWD1X1_RING, P.FWD1X1_RING + 1} <= pers
    assert max(pers) > 2 * P.FWD1X1_RING                           # the ring wraps twice
    first, last5 = P.FWD1X1_CASES[0], P.FWD1X1_CASES[4]
    assert P.FWD1X1_CAP - -(-first.total // first.per) == 255       # 255 workgroups with an empty range
    assert empties > 255 and short_last >= 4 and crossing == len(P.FWD1X1_CASES) - 1
    assert last5.total % last5.per == 3                             # last non-empty range: 3 items
    ragged = {c.H * c.W % P.FWD1X1_ITEM_PX for c in P.FWD1X1_CASES}
    assert {0, 1, 3, 15} <= ragged                                  # full, 1-pixel, 3-pixel items; 15 of 32 in every item
    assert {c.res for c in P.FWD1X1_CASES} == {None, "plain", "virtual"} and {c.relu for c in P.FWD1X1_CASES} == {0, 1}
    assert {c.cin for c in P.FWD1X1_CASES} == {256, 128}


def test_dgrad1x1_cases_reach_the_unrolled_tail_and_empty_workgroups():
    from tactilesr_amd import _lib
    lib = _lib.load()
    pers, tails, crossing = set(), set(), 0
    for c in P.DGRAD1X1_CASES:
        gpi = -(-(c.H * c.W) // P.DGRAD1X1_GROUP_PX)
        grid, per, rng = _ranges(c.B * gpi, P.DGRAD1X1_CAP)
        assert (c.B * gpi, per) == (c.total, c.per), c
        assert lib.tsr_conv2d_slab_entries_ex(c.B, c.H, c.W, P.DG_N, 1, -3) == grid == 2048
        pers.add(per)
        tails |= {(b - a) % P.DGRAD1X1_U for a, b in rng if b > a}
        crossing += any(a // gpi != (b - 1) // gpi for a, b in rng if b > a)
    assert pers == {2, 3, 5, 9} and crossing == len(P.DGRAD1X1_CASES) - 1      # (per 3 = groups per image: one image each)
    assert tails == {1, 2, 3}                                       # every partial fill of the last block of U = 4 groups,
    assert max(pers) > 2 * P.DGRAD1X1_U                             # behind up to two full blocks
    first = P.DGRAD1X1_CASES[0]
    assert P.DGRAD1X1_CAP - -(-first.total // first.per) == 1023    # 1023 workgroups with an empty range
    assert {c.ci0 for c in P.DGRAD1X1_CASES} == {0, 128} and sum(c.also_without_bn for c in P.DGRAD1X1_CASES) == 1
    t = torch.arange(2 * 3 * 5 * 7, dtype=torch.float64).view(2, 3, 5, 7)
    s = P.entry_sums(t, 4, 2)                                       # 6 groups of 16, 16, 3 pixels on 4 entries of 2
    assert torch.equal(s.sum(0), t.sum(dim=(0, 2, 3))) and float(s[3].abs().max()) == 0
    assert torch.equal(s[1], t[0].reshape(3, 35)[:, 32:].sum(1) + t[1].reshape(3, 35)[:, :16].sum(1))


def test_conv1x1_b16_ex_cases_pass_the_grid_once():
    for c in P.STREAM1X1_CASES:
        tiles = -(-c.H // 8) * -(-c.W // 8)
        total = -(-c.B // 4) * tiles
        assert total == c.total and P.STREAM1X1_CAP < total < 2 * P.STREAM1X1_CAP      # workgroup 0 takes items 0 and 512
        assert c.B % 4 in (1, 2)                                    # the last image group is not full
    assert {(c.H, c.W, c.B, c.res) for c in P.STREAM1X1_CASES} == {(5, 7, 2049, "plain"), (5, 7, 2049, None),
                                                                   (9, 7, 1030, "plain"), (9, 7, 1030, None)}


def test_tpsf_indices_lie_in_later_iterations_of_every_grid():
    idx = P.TPSF_INDICES
    assert len(idx) == len(set(idx)) == 24 and max(idx) == P.TPSF_B - 1
    assert {0, 255, 256, 511, 512, 513, 767, 768, 1024, 2047, 2048, 2099} <= set(idx)
    for grid in (P.TPSF_FWD_GRID, P.TPSF_DHB_GRID, P.TPSF_POOL_GRID):
        later = [b for b in idx if b >= grid]
        assert later and grid % 5 != 0                              # a workgroup's consecutive samples differ in scale
        assert max(b // grid for b in idx) == (P.TPSF_B - 1) // grid        # and its LAST iteration is compared too
    assert {b // P.TPSF_FWD_GRID for b in idx} == {0, 1, 2, 3, 4}
    assert {b // P.TPSF_DHB_GRID for b in idx} == set(range(9))
    depth, ab, dl = P.tpsf_inputs()
    assert depth.shape == (P.TPSF_B, 100, 100) and ab.shape == (P.TPSF_B, 3) and dl.shape == (P.TPSF_B, 16)
    assert float(depth[P.TPSF_ZERO].abs().max()) == 0 and float(depth[P.TPSF_SIGNED].min()) < 0 < float(depth[P.TPSF_SIGNED].max())
    pl = depth[P.TPSF_PLATEAU]
    assert int((pl == pl.max()).sum()) == 625 and int((pl == 0).sum()) == 10000 - 625
    mx = depth.abs().amax(dim=(1, 2))
    assert float(mx[1025] / mx[1024]) < 1e-3 and float(mx[514] / mx[513]) > 5      # orders of magnitude between neighbours


def test_output_bar_rejects_one_item_served_from_the_previous_slot():
    """The largest forward case (B = 2049: 4.6 million outputs): bf16(ref) passes; with ONE 32-pixel item (0.04 % of the
    outputs, far inside the 1 % that may differ) replaced by its predecessor -- the other item of its image, or the last
    item of the image before, which differs by a power of two -- the bar rejects it: no element may be beyond one ulp."""
    c = P.FWD1X1_CASES[4]
    ref = P.fwd_inputs(c)["ref"]
    good = q16(ref.float())
    assert "beyond one ulp 0" in check_tensor(-1, good, ref)
    ipi = -(-(c.H * c.W) // P.FWD1X1_ITEM_PX)
    for item in (c.per, c.per + 1, c.total - 1):         # first item of workgroup 1's range (mid-image), its second, the last
        bad = P.swap_item_for_predecessor(good, item, ipi)
        assert int((bad != good).sum()) <= 32 * P.COUT
        with pytest.raises(AssertionError, match="beyond one ulp"):
            check_tensor(-1, bad, ref)
