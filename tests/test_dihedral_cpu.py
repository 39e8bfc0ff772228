"""CPU side of the rot90 / flip augmentation (tests/_dihedral_cases.py): the restatement is np.rot90, the host tables
compose and invert as the transforms do, the vector axis mode is the op's coordinate matrix, the entry point is declared
and bound at ABI 24, every refusal is refused before any device call, and the loader / data helpers on device="cpu"
do what the reference's augmentData does -- while augment=None stays today's loader, generator state included."""
import os
import re

import numpy as np
import pytest
import torch

import _dihedral_cases as DC
from tactilesr_amd import _lib
from tactilesr_amd import data as D
from tactilesr_amd import functional as Fh
from tactilesr_amd.data import DeviceSRLoader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(mode, C):
    return DC.axis_tables(C) if mode == "vector" else None


def test_restatement_is_np_rot90_per_plane():
    x = DC.make_src(3, (3, 5, 5), 11)
    for k in range(4):
        got = DC.restate(x, [k] * 3)
        for b in range(3):
            for c in range(3):
                want = np.rot90(x[b, c].numpy(), k)
                assert np.array_equal(got[b, c].numpy(), want), (k, b, c)
    # the mirrored half: the mirror along W first, then the same turns
    for k in range(4):
        got = DC.restate(x, [k + 4] * 3)
        want = np.rot90(x.numpy()[..., ::-1], k, axes=(-2, -1))
        assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("mode", ["planes", "vector"])
def test_functional_torch_path_equals_the_restatement(mode):
    x = DC.make_src(9, (6, 4, 4), 12)
    ops = DC.make_ops(9, DC.OPS, 13)
    idx = DC.make_index("repeats", 9, 9, 14)
    got = Fh.dihedral(x, torch.tensor(ops, dtype=torch.int32), idx, axis_mode=mode)
    DC.assert_same_bits(got, DC.restate(x, ops, idx, _tables(mode, 6)), mode)
    for op in DC.OPS:
        DC.assert_same_bits(Fh.dihedral(x, op_all=op, axis_mode=mode), DC.restate(x, [op] * 9, None, _tables(mode, 6)), op)
    y = DC.make_src(4, (1, 3, 7), 15)[:, 0]                         # (N, H, W), even k on a non-square plane
    DC.assert_same_bits(Fh.dihedral(y, [0, 2, 4, 6]), DC.restate(y.unsqueeze(1), [0, 2, 4, 6])[:, 0])
    prior = DC.make_src(9, (6, 4, 4), 16)
    out = prior.clone()
    res = Fh.dihedral(x, ops, idx, out=out, scale=-0.25, accumulate=True, axis_mode=mode)
    assert res is out
    want = prior.double() - 0.25 * DC.restate(x, ops, idx, _tables(mode, 6)).double()
    assert float((out.double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())


def test_index_sequences_and_overlapping_out():
    x = DC.make_src(6, (3, 4, 4), 17)
    want = DC.restate(x, [1, 6, 3], [4, 0, 4])
    DC.assert_same_bits(Fh.dihedral(x, [1, 6, 3], [4, 0, 4]), want)                       # sequences for both
    DC.assert_same_bits(Fh.dihedral(x, (1, 6, 3), torch.tensor([4, 0, 4], dtype=torch.int32)), want)
    DC.assert_same_bits(Fh.dihedral(x[:, 0], [1, 6, 3], (4, 0, 4)), want[:, 0])
    with pytest.raises(_lib.TactileSRHipError):
        Fh.dihedral(x, [1, 6], [[4, 0]])
    big = DC.make_src(12, (3, 4, 4), 18)
    for out in (big[:6], big[3:9], big[5:11]):                                          # x itself, and both partial overlaps
        with pytest.raises(_lib.TactileSRHipError):
            Fh.dihedral(big[3:9], op_all=2, out=out)
    with pytest.raises(_lib.TactileSRHipError):
        Fh.dihedral(big.transpose(2, 3)[:6], op_all=0, out=big[6:])                      # a strided view of out's storage
    got = Fh.dihedral(big[:6], op_all=2, out=big[6:])                                    # neighbours in one allocation are fine
    DC.assert_same_bits(got, DC.restate(big[:6], [2] * 6))
    with pytest.raises(TypeError):
        Fh.dihedral(x, None, None, None, 1.0, False, "planes", 0, 0xff)                   # the extras are keyword-only


def test_host_tables_match_the_axis_tables_of_the_restatement():
    for C, ac in ((3, 3), (24, 3), (6, 2), (8, 4)):
        cmap, csign = Fh.dihedral_axis_tables(C, ac)
        rc, rs = DC.axis_tables(C, ac)
        assert cmap.dtype == torch.int32 and csign.dtype == torch.float32 and cmap.shape == csign.shape == (8, C)
        assert torch.equal(cmap, rc) and torch.equal(csign, rs), (C, ac)
    for bad in ((4, 3), (3, 1), (0, 3)):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.dihedral_axis_tables(*bad)


@pytest.mark.parametrize("mode", ["planes", "vector"])
def test_compose_equals_two_ops_in_turn(mode):
    x = DC.make_src(2, (3, 5, 5), 21)
    t = _tables(mode, 3)
    for a in DC.OPS:
        first = DC.restate(x, [a] * 2, None, t)
        for b in DC.OPS:
            c = Fh.dihedral_compose(a, b)
            DC.assert_same_bits(DC.restate(first, [b] * 2, None, t), DC.restate(x, [c] * 2, None, t), (a, b, c))


@pytest.mark.parametrize("mode", ["planes", "vector"])
def test_op_then_inverse_is_the_identity(mode):
    x = DC.make_src(2, (3, 6, 6), 22)
    t = _tables(mode, 3)
    for op in DC.OPS:
        inv = Fh.dihedral_inverse(op)
        assert Fh.dihedral_compose(op, inv) == 0 and Fh.dihedral_compose(inv, op) == 0
        DC.assert_same_bits(DC.restate(DC.restate(x, [op] * 2, None, t), [inv] * 2, None, t), x, op)
    assert [Fh.dihedral_inverse(o) for o in DC.OPS] == [0, 3, 2, 1, 4, 5, 6, 7]
    for bad in (8, -1, 1.5):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.dihedral_inverse(bad)


def test_vector_mode_geometry():
    cmap, csign = Fh.dihedral_axis_tables(6, 3)
    for op in DC.OPS:
        for g in (0, 3):
            assert int(cmap[op, g + 2]) == g + 2 and float(csign[op, g + 2]) == 1.0        # the normal never moves
            swapped = (int(cmap[op, g]), int(cmap[op, g + 1])) == (g + 1, g)
            assert swapped == bool(op & 1)                                             # a quarter turn swaps the pair
            if not swapped:
                assert (int(cmap[op, g]), int(cmap[op, g + 1])) == (g, g + 1)
            d = float(csign[op, g] * csign[op, g + 1]) * (-1.0 if swapped else 1.0)
            assert d == DC.det(op) == (-1.0 if op >= 4 else 1.0), op                   # exactly the mirrors flip handedness
    assert torch.equal(cmap[0], torch.arange(6, dtype=torch.int32)) and bool((csign[0] == 1).all())
    # a force along +W (to the right), turned a quarter counter-clockwise, points up: -H
    x = torch.zeros(1, 3, 4, 4)
    x[0, 1] = 2.0
    y = Fh.dihedral(x, op_all=1, axis_mode="vector")
    assert bool((y[0, 0] == -2.0).all()) and bool((y[0, 1] == 0).all())


def test_symbol_declared_bound_and_exported_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    decl = re.search(r"^int\s+tsr_gather_dihedral\s*\(([^;]*)\)\s*;", header, re.M)
    assert decl, "tsr_gather_dihedral is not declared in include/tactilesr_hip.h"
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["tsr_gather_dihedral"]) == 16
    para = header[header.index("Rot90 / flip augmentation on the device"):decl.start()]
    assert "out[b] = (accumulate ? out[b] : 0) + scale * D_{op[b]}( src[ idx ? idx[b] : b ] )" in para
    assert "Refusals" in para and "2^31 - 1" in para
    lib = _lib.load()
    assert hasattr(lib, "tsr_gather_dihedral")
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24
    wgs = re.search(r"^int\s+tsr_gather_dihedral_wgs\s*\(([^;]*)\)\s*;", header, re.M)
    assert wgs and len(wgs.group(1).split(",")) == len(_lib.SIGNATURES["tsr_gather_dihedral_wgs"]) == 17
    cap = re.search(r"^#define\s+TSR_DIHEDRAL_MAX_WGS\s+\(1 << (\d+)\)", header, re.M)
    assert cap and int(cap.group(1)) == 20 and DC.WALKS[-1][0] == 1 << 20 and hasattr(lib, "tsr_gather_dihedral_wgs")
    declared = set(re.findall(r"^(?:int|long long)\s+(\w+)\s*\(", header, re.M))
    assert declared == set(_lib.SIGNATURES)
    src = open(os.path.join(REPO, "tactilesr_amd", "csrc", "dihedral.hip")).read()
    assert "getenv" not in src and "asm" not in src and "atomic" not in src.replace("No atomics", "")


@pytest.mark.parametrize("label,over", DC.REFUSALS, ids=[r[0] for r in DC.REFUSALS])
def test_refusals_need_no_device(label, over):
    """Status 1 before any device call: the pointers are small fake addresses nothing may dereference."""
    assert DC.call_raw(_lib.load(), dict(DC.BASE_ARGS, **over)) == 1, label


def test_shape_tables_reach_every_kernel_and_both_sides_of_each_threshold():
    src = open(os.path.join(REPO, "tactilesr_amd", "csrc", "dihedral.hip")).read()
    assert int(re.search(r"DH_PLANE_LDS\s*=\s*(\d+)", src).group(1)) == DC.PLANE_LDS_DWORDS
    assert int(re.search(r"DH_SMALL\s*=\s*(\d+)", src).group(1)) == 64
    shapes = [s for s, _ in DC.SHAPES + DC.NONSQUARE]
    assert {DC.path_of(s) for s in shapes} == {"small", "plane", "tile"}
    assert DC.path_of((1, 8, 8)) == "small" and DC.path_of((1, 9, 9)) == "plane"
    assert DC.path_of((1, 125, 125)) == "plane" and DC.path_of((1, 126, 126)) == "tile"
    for path in ("plane", "tile"):                                  # float4 rows and one float per lane, on both
        assert {s[2] % 4 == 0 for s in shapes if DC.path_of(s) == path} == {True, False}
    assert all(DC.path_of(s) == "plane" for s in ((1, 40, 40), (1, 100, 100), (1, 124, 124)))   # the project's shapes
    assert all(why for _, why in DC.SHAPES + DC.NONSQUARE)


def test_refusal_table_covers_the_contract():
    keys = {k for _, over in DC.REFUSALS for k in over}
    assert keys >= {"src", "out", "B", "n_src", "C", "H", "W", "op_mask", "op", "op_all", "cmap", "csign", "accumulate", "scale"}


# ---- the loader on device="cpu"
def _set(n=10, seed=31):
    return DC.make_src(n, (3, 4, 4), seed), DC.make_src(n, (1, 12, 12), seed + 1)[:, 0]


def test_loader_without_augment_is_todays_loader():
    LR, HR = _set()
    for shuffle in (False, True):
        a = DeviceSRLoader(LR, HR, 4, shuffle=shuffle, seed=5, device="cpu")
        b = DeviceSRLoader(LR, HR, 4, shuffle=shuffle, seed=5, device="cpu", augment=None, augment_mode="expand",
                           axis_mode="vector")
        g = torch.Generator().manual_seed(5)                        # the loader as it was: one randperm per epoch
        for _ in range(2):
            order = torch.randperm(10, generator=g) if shuffle else torch.arange(10)
            got_a, got_b = list(a), list(b)
            assert len(got_a) == len(got_b) == len(a) == len(b) == 3
            for i, ((la, ha), (lb, hb)) in enumerate(zip(got_a, got_b)):
                idx = order[4 * i:4 * i + 4]
                DC.assert_same_bits(la, LR[idx]), DC.assert_same_bits(ha, HR[idx])
                DC.assert_same_bits(lb, LR[idx]), DC.assert_same_bits(hb, HR[idx])
        assert torch.equal(a._gen.get_state(), g.get_state()) and torch.equal(b._gen.get_state(), g.get_state())
        assert b.last_index is None and b.last_ops is None


def test_loader_expand_unshuffled_is_augment_arrays_order():
    LR, HR = _set()
    aLR, aHR = D.augment_arrays(LR.numpy(), HR.numpy())
    assert aLR.shape == (40, 3, 4, 4) and aHR.shape == (40, 12, 12)
    ld = DeviceSRLoader(LR, HR, 7, device="cpu", augment="rot90", augment_mode="expand")
    assert len(ld) == 6
    got = list(ld)
    DC.assert_same_bits(torch.cat([g[0] for g in got]), torch.from_numpy(aLR))
    DC.assert_same_bits(torch.cat([g[1] for g in got]), torch.from_numpy(aHR))
    assert ld.last_index.tolist() == [8, 9, 9, 9, 9] and ld.last_ops.tolist() == [3, 0, 1, 2, 3]
    assert len(DeviceSRLoader(LR, HR, 7, device="cpu", augment="dihedral", augment_mode="expand", drop_last=True)) == 11
    # shuffled: every (sample, op) pair exactly once
    sh = DeviceSRLoader(LR, HR, 7, device="cpu", augment=(0, 2, 5), augment_mode="expand", shuffle=True, seed=3)
    pairs = []
    for l, h in sh:
        pairs += list(zip(sh.last_index.tolist(), sh.last_ops.tolist()))
        DC.assert_same_bits(l, DC.restate(LR, sh.last_ops.tolist(), sh.last_index))
        DC.assert_same_bits(h, DC.restate(HR.unsqueeze(1), sh.last_ops.tolist(), sh.last_index)[:, 0])
    assert sorted(pairs) == [(s, o) for s in range(10) for o in (0, 2, 5)]


@pytest.mark.parametrize("mode", ["planes", "vector"])
def test_loader_random_keeps_pairs_aligned_and_is_reproducible(mode):
    LR, HR = _set(23, 41)
    HR4 = HR.unsqueeze(1)                                           # the (N,1,H,W) form of the second tensor

    def epoch(ld):
        out = []
        for l, h in ld:
            out.append((l.clone(), h.clone(), ld.last_index.clone(), ld.last_ops.clone()))
        return out
    a = DeviceSRLoader(LR, HR4, 8, shuffle=True, seed=9, device="cpu", augment="dihedral", axis_mode=mode)
    b = DeviceSRLoader(LR, HR4, 8, shuffle=True, seed=9, device="cpu", augment="dihedral", axis_mode=mode)
    assert len(a) == 3
    e1, e2, f1 = epoch(a), epoch(a), epoch(b)
    seen, samples = set(), []
    for (l, h, idx, ops), (l2, h2, idx2, ops2) in zip(e1, f1):
        assert torch.equal(idx, idx2) and torch.equal(ops, ops2)
        DC.assert_same_bits(l, l2), DC.assert_same_bits(h, h2)
        assert ops.dtype == torch.int32 and idx.dtype == torch.int64 and h.shape[1:] == (1, 12, 12)
        DC.assert_same_bits(l, DC.restate(LR, ops.tolist(), idx, _tables(mode, 3)))
        DC.assert_same_bits(h, DC.restate(HR4, ops.tolist(), idx))              # the same op on both tensors of a pair
        seen |= set(ops.tolist())
        samples += idx.tolist()
    assert sorted(samples) == list(range(23)) and len(seen) >= 5
    assert any(not torch.equal(x[3], y[3]) for x, y in zip(e1, e2))             # a fresh draw per epoch
    # the draws: the permutation first, then one op index per sample, from the loader's own generator
    g = torch.Generator().manual_seed(9)
    order = torch.randperm(23, generator=g)
    draw = torch.randint(0, 8, (23,), generator=g)
    assert torch.equal(torch.cat([x[2] for x in e1]), order) and torch.equal(torch.cat([x[3] for x in e1]).long(), draw)


def test_loader_argument_checks():
    LR, HR = _set()
    wide = torch.zeros(10, 12, 14)
    for kw in (dict(augment="rot90"), dict(augment=(0, 3)), dict(augment="dihedral", augment_mode="expand")):
        with pytest.raises(_lib.TactileSRHipError):
            DeviceSRLoader(LR, wide, 4, device="cpu", **kw)
    ld = DeviceSRLoader(LR, wide, 4, device="cpu", augment=(0, 2, 4, 6))        # even k: any shape
    l, h = next(iter(ld))
    assert h.shape == (4, 12, 14)
    for kw in (dict(augment="rot45"), dict(augment=()), dict(augment=(0, 0)), dict(augment=(8,)),
               dict(augment="rot90", augment_mode="both"), dict(augment="rot90", axis_mode="tensor")):
        with pytest.raises(_lib.TactileSRHipError):
            DeviceSRLoader(LR, HR, 4, device="cpu", **kw)
    sharded = DeviceSRLoader(LR, HR, 4, device="cpu", augment="rot90", augment_mode="expand", rank=1, world_size=3)
    assert sharded.LR.shape[0] == 4 and len(sharded) == 4                       # ceil(10 / 3) base samples, times 4 ops


def test_tpsf_loader_honours_is_aug_data():
    from tactilesr_amd.config.default import tPSFNet_config
    LR, HR = _set()
    assert tPSFNet_config["is_aug_data"] is False
    plain = D.tpsf_loader(LR.numpy(), HR.numpy(), tPSFNet_config, 4, device="cpu")
    assert plain._ops is None and len(plain) == 3
    aug = D.tpsf_loader(LR, HR, dict(tPSFNet_config, is_aug_data=True), 4, device="cpu")
    assert aug._ops == (0, 1, 2, 3) and aug.augment_mode == "expand" and len(aug) == 10
    aLR, aHR = D.augment_arrays(LR, HR)
    DC.assert_same_bits(torch.cat([b[0] for b in aug]), torch.from_numpy(aLR))
    assert D.tpsf_loader(LR, HR, {}, 4, device="cpu")._ops is None
    rnd = D.tpsf_loader(LR, HR, dict(is_aug_data=True), 4, device="cpu", augment_mode="random", shuffle=True)
    assert rnd.augment_mode == "random" and len(rnd) == 3


def test_augment_arrays_equals_the_reference(golden):
    g = golden("augment")
    aLR, aHR = D.augment_arrays(g["LR"], g["depth"])
    assert aLR.dtype == np.float32 and aLR.shape == g["aug_LR"].shape == (20, 3, 4, 4)
    assert aHR.shape == g["aug_depth"].shape == (20, 100, 100)
    assert np.array_equal(aLR.view(np.int32), g["aug_LR"].view(np.int32))
    assert np.array_equal(aHR.view(np.int32), g["aug_depth"].view(np.int32))
    # and the restatement's ops 0..3 are the reference's four, in its order
    ops = [0, 1, 2, 3] * 5
    idx = torch.arange(5).repeat_interleave(4)
    DC.assert_same_bits(DC.restate(torch.from_numpy(g["LR"]), ops, idx), torch.from_numpy(g["aug_LR"]))
    DC.assert_same_bits(DC.restate(torch.from_numpy(g["depth"]).unsqueeze(1), ops, idx)[:, 0], torch.from_numpy(g["aug_depth"]))


def test_self_ensemble_and_eval_keyword_exist():
    import inspect
    from tactilesr_amd.train import tactileSR_train as TR
    assert inspect.signature(TR.eval_func).parameters["self_ensemble"].default is None
    assert Fh.dihedral_ops("rot90") == (0, 1, 2, 3) and Fh.dihedral_ops("dihedral") == tuple(range(8))
    sig = inspect.signature(Fh.dihedral).parameters
    assert [sig[k].default for k in ("ops", "index", "out", "scale", "accumulate", "axis_mode", "op_all")] == \
        [None, None, None, 1.0, False, "planes", 0]
    for fn in (Fh.dihedral, Fh.self_ensemble, DeviceSRLoader):
        assert "autograd" in fn.__doc__ or "differentiable" in fn.__doc__
