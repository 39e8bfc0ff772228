"""GPU checks of the rot90 / flip augmentation (tsr_gather_dihedral, functional.dihedral / self_ensemble, the augmenting
DeviceSRLoader, eval_func's self-ensemble) against the torch restatement of tests/_dihedral_cases.py, bit for bit.
Every launch writes into a NaN-prefilled output between NaN guard bands, reads a source that is a slice of a larger
allocation with one guard sample on either side, and runs twice: the two runs must give the same bits."""
import pytest
import torch

import _dihedral_cases as DC
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib, optim
from tactilesr_amd.data import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _placed(n, off, guard, fill=None):
    """n floats starting `off` floats past a 16-byte boundary inside a NaN-filled device buffer, with at least `guard`
    NaN floats on either side: (buffer, the view, its start)."""
    start = (guard + 3) // 4 * 4 + off
    buf = torch.full((start + n + guard + 4,), NAN, dtype=torch.float32, device="cuda")
    mid = buf[start:start + n]
    assert mid.data_ptr() % 16 == 4 * off
    if fill is not None:
        mid.copy_(fill.reshape(-1))
    return buf, mid, start


def _launch(src, B, ops=None, index=None, op_all=0, op_mask=None, tables=None, scale=1.0, accumulate=0, prior=None,
            src_off=0, out_off=0, expect=0, max_wgs=None):
    """One raw launch (twice, into two fresh buffers): the (B,C,H,W) output on the CPU.  ``src`` is a CPU tensor."""
    n_src, C, H, W = src.shape
    chw = C * H * W
    guard = max(chw, 64)
    _, sd, _ = _placed(n_src * chw, src_off, guard, src.cuda())
    od = None if ops is None else torch.tensor(ops, dtype=torch.int32, device="cuda")
    idd = None if index is None else torch.as_tensor(index, dtype=torch.int64).cuda()
    cm, cs = (None, None) if tables is None else (tables[0].cuda().contiguous(), tables[1].cuda().contiguous())
    if op_mask is None:
        op_mask = DC.mask_of(ops) if ops is not None else 1 << op_all
    a = dict(n_src=n_src, op_all=op_all, op_mask=op_mask, B=B, C=C, H=H, W=W, scale=scale, accumulate=accumulate)
    if max_wgs is not None:
        a["max_wgs"] = max_wgs                                  # tsr_gather_dihedral_wgs
    outs = []
    for _ in range(2):
        obuf, out, start = _placed(B * chw, out_off, guard, None if prior is None else prior.cuda())
        st = DC.call_raw(_lib.load(), a, stream=torch.cuda.current_stream().cuda_stream, src=sd.data_ptr(),
                         idx=0 if idd is None else idd.data_ptr(), op=0 if od is None else od.data_ptr(),
                         cmap=0 if cm is None else cm.data_ptr(), csign=0 if cs is None else cs.data_ptr(),
                         out=out.data_ptr())
        assert st == expect, st
        torch.cuda.synchronize()
        assert bool(torch.isnan(obuf[:start]).all() and torch.isnan(obuf[start + B * chw:]).all()), "guard band written"
        outs.append(out.cpu().view(B, C, H, W))
    DC.assert_same_bits(outs[0], outs[1], "two launches")
    return outs[0]


def _modes(C):
    return (("planes", None), ("vector", DC.axis_tables(C))) if C % 3 == 0 else (("planes", None),)


ALL_SHAPES = [(s, DC.OPS) for s, _ in DC.SHAPES] + [(s, DC.EVEN_OPS) for s, _ in DC.NONSQUARE]


@pytest.mark.parametrize("B", DC.BATCHES)
@pytest.mark.parametrize("shape,allowed", ALL_SHAPES, ids=["x".join(map(str, s)) for s, _ in ALL_SHAPES])
def test_every_shape_batch_and_index(shape, allowed, B):
    n_src = B + 3
    src = DC.make_src(n_src, shape, 100 + B)
    ops = DC.make_ops(B, allowed, 200 + B)
    if B >= len(allowed):
        assert set(ops) == set(allowed)
    for kind in DC.INDEX_KINDS:
        index = DC.make_index(kind, B, n_src, 300 + B)
        for mode, tables in _modes(shape[0]):
            got = _launch(src, B, ops, index, tables=tables)
            DC.assert_same_bits(got, DC.restate(src[:B] if index is None else src, ops, index, tables), (kind, mode))


@pytest.mark.parametrize("shape", [(3, 4, 4), (1, 40, 40), (1, 100, 100), (1, 65, 65), (1, 132, 132)], ids=str)
def test_bases_off_alignment(shape):
    src = DC.make_src(9, shape, 41)
    ops = DC.make_ops(7, DC.OPS, 42)
    index = DC.make_index("perm", 7, 9, 43)
    want = DC.restate(src, ops, index)
    for so in (0,) + DC.OFFSETS:
        for oo in (0,) + DC.OFFSETS:
            if so or oo:
                DC.assert_same_bits(_launch(src, 7, ops, index, src_off=so, out_off=oo), want, (so, oo))


@pytest.mark.parametrize("shape,allowed", [((3, 4, 4), DC.OPS), ((1, 40, 40), DC.OPS), ((2, 33, 33), DC.OPS),
                                           ((1, 132, 132), DC.OPS), ((3, 5, 7), DC.EVEN_OPS), ((1, 31, 65), DC.EVEN_OPS),
                                           ((1, 36, 500), DC.EVEN_OPS)], ids=str)
def test_one_op_for_all_samples(shape, allowed):
    src = DC.make_src(5, shape, 51)
    index = DC.make_index("reversed", 4, 5, 52)
    for op in allowed:
        for mode, tables in _modes(shape[0]):
            want = DC.restate(src, [op] * 4, index, tables)
            DC.assert_same_bits(_launch(src, 4, None, index, op_all=op, tables=tables), want, (op, mode))
            DC.assert_same_bits(_launch(src, 4, None, index, op_all=op, op_mask=DC.mask_of(allowed), tables=tables), want)
            DC.assert_same_bits(_launch(src, 5, None, None, op_all=op, tables=tables), DC.restate(src, [op] * 5, None, tables))


WALK_SHAPES = [((24, 4, 4), DC.OPS, 30), ((1, 40, 40), DC.OPS, 9), ((2, 33, 33), DC.OPS, 9), ((1, 132, 132), DC.OPS, 5),
               ((1, 129, 129), DC.OPS, 5), ((1, 36, 500), DC.EVEN_OPS, 3)]


@pytest.mark.parametrize("max_wgs", [w for w, _ in DC.WALKS])
@pytest.mark.parametrize("shape,allowed,B", WALK_SHAPES, ids=[str(s) for s, _, _ in WALK_SHAPES])
def test_capped_grids_walk_to_the_same_bits(shape, allowed, B, max_wgs):
    """Every kernel with 1, 3 and the default number of workgroups: each workgroup walks several elements, planes or
    tiles (45 / 9 / 18 / 45 / 45 / 24 items here), transposing ones and an all-NaN one among them."""
    src = DC.make_src(B + 2, shape, 161)
    ops = DC.make_ops(B, allowed, 162)
    index = DC.make_index("perm", B, B + 2, 163)
    want = DC.restate(src, ops, index)
    DC.assert_same_bits(_launch(src, B, ops, index, max_wgs=max_wgs), want)
    bad = list(ops)
    bad[1] = 8                                                       # a NaN sample in the middle of a walk
    got = _launch(src, B, bad, index, op_mask=DC.mask_of(allowed), max_wgs=max_wgs)
    for b in range(B):
        if b == 1:
            assert bool(torch.isnan(got[b]).all())
        else:
            DC.assert_same_bits(got[b], want[b], b)
    prior = DC.make_src(B, shape, 164)
    got = _launch(src, B, ops, index, scale=0.5, accumulate=1, prior=prior, max_wgs=max_wgs)
    assert torch.equal(got, torch.addcmul(prior, want, torch.tensor(0.5)))              # 0.5 x is exact: one rounding
    _launch(src, B, ops, index, max_wgs=0, expect=1)                 # refused: the output keeps its NaN prefill


def test_many_distinct_samples():
    n, shape = DC.MANY
    src = DC.make_src(n, shape, 61)
    ops = DC.make_ops(n, DC.OPS, 62)
    index = DC.make_index("perm", n, n, 63)
    DC.assert_same_bits(_launch(src, n, ops, index), DC.restate(src, ops, index))


@pytest.mark.parametrize("shape", [(3, 4, 4), (1, 40, 40), (2, 33, 33), (1, 132, 132)], ids=str)
def test_nonfinite_elements_arrive_bit_for_bit(shape):
    src = DC.make_src(6, shape, 71)
    specials = torch.tensor([0x7fc00000, 0x7fc12345, -0x3fffff, 0x7f800001, 0x7f800000, -0x800000, -0x80000000],
                            dtype=torch.int32)                      # NaNs with payloads and signs, a signalling one, +-Inf, -0
    flat = src.view(torch.int32).view(-1)
    g = torch.Generator().manual_seed(72)
    where = torch.randperm(flat.numel(), generator=g)[:4 * len(specials)]
    flat[where] = specials.repeat(4)
    assert int(torch.isnan(src).sum()) == 16
    ops = DC.make_ops(8, DC.OPS, 73)
    index = DC.make_index("repeats", 8, 6, 74)
    for mode, tables in _modes(shape[0]):
        want = DC.restate(src, ops, index, tables)
        got = _launch(src, 8, ops, index, tables=tables)
        DC.assert_same_bits(got, want, mode)
        if tables is None:                                          # a pure move: the multiset of bit patterns per plane is kept
            sel = src.index_select(0, index)
            assert torch.equal(DC.bits(got).view(8, shape[0], -1).sort(-1)[0], DC.bits(sel).view(8, shape[0], -1).sort(-1)[0])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", [(3, 4, 4), (1, 40, 40), (1, 65, 65), (1, 132, 132), (1, 129, 129)], ids=str)
def test_bad_device_values_give_nan_samples_only(shape, accumulate):
    n_src, B = 5, 8
    src = DC.make_src(n_src, shape, 81)
    good_ops = [0, 1, 2, 3, 0, 2, 1, 3]
    good_idx = [0, 1, 2, 3, 4, 0, 4, 2]
    prior = DC.make_src(B, shape, 82) if accumulate else None
    scale = 0.5 if accumulate else 1.0
    clean = _launch(src, B, good_ops, good_idx, op_mask=0x0f, scale=scale, accumulate=accumulate, prior=prior)
    want = DC.restate(src, good_ops, good_idx)
    if accumulate:
        assert torch.equal(clean, torch.addcmul(prior, want, torch.tensor(0.5)))        # 0.5 x is exact: one rounding either way
    else:
        DC.assert_same_bits(clean, want)
    ops, idx = list(good_ops), list(good_idx)
    ops[1], ops[3], ops[5] = 8, 5, -1                                # outside 0..7, outside op_mask (0x0f), negative
    idx[2], idx[4] = -1, n_src                                       # the guard samples on either side
    got = _launch(src, B, ops, idx, op_mask=0x0f, scale=scale, accumulate=accumulate, prior=prior)
    for b in range(B):
        if b in (1, 2, 3, 4, 5):
            assert bool(torch.isnan(got[b]).all()), b
        else:
            DC.assert_same_bits(got[b], clean[b], b)
    # without idx the sample number is the source index: rows past n_src are NaN, the others whole
    got = _launch(src, B, good_ops, None, op_mask=0x0f)
    DC.assert_same_bits(got[:n_src], DC.restate(src, good_ops[:n_src]))
    assert bool(torch.isnan(got[n_src:]).all())
    # a channel map entry outside [0, C) spoils its plane of every sample that uses the op, nothing else
    if shape[0] == 3:
        cmap, csign = DC.axis_tables(3)
        cmap = cmap.clone()
        cmap[2, 1] = 3
        got = _launch(src, B, good_ops, good_idx, op_mask=0x0f, tables=(cmap, csign))
        want = DC.restate(src, good_ops, good_idx, DC.axis_tables(3))
        for b in range(B):
            for c in range(3):
                if good_ops[b] == 2 and c == 1:
                    assert bool(torch.isnan(got[b, c]).all())
                else:
                    DC.assert_same_bits(got[b, c], want[b, c], (b, c))


@pytest.mark.parametrize("shape", [(3, 4, 4), (1, 40, 40), (1, 65, 65), (3, 5, 7), (1, 132, 132), (1, 129, 129)], ids=str)
def test_scale_and_accumulate_against_fp64(shape):
    allowed = DC.OPS if shape[1] == shape[2] else DC.EVEN_OPS
    src = DC.make_src(9, shape, 91) * (1.0 / 3.0)                    # values with full mantissas
    prior = DC.make_src(8, shape, 92) * (1.0 / 7.0)
    ops = DC.make_ops(8, allowed, 93)
    index = DC.make_index("perm", 8, 9, 94)
    for mode, tables in _modes(shape[0]):
        x = DC.restate(src, ops, index, tables)
        for scale in DC.SCALES:
            sx = scale * x.double()
            got = _launch(src, 8, ops, index, tables=tables, scale=scale, accumulate=1, prior=prior)
            err = (got.double() - (prior.double() + sx)).abs()
            bound = 2.0 ** -23 * (prior.double().abs() + sx.abs())
            assert bool((err <= bound).all()), (mode, scale, float((err - bound).max()))
            got = _launch(src, 8, ops, index, tables=tables, scale=scale)
            if scale == 1.0:
                DC.assert_same_bits(got, x, mode)                    # the copying form
            else:
                assert bool(((got.double() - sx).abs() <= 2.0 ** -23 * sx.abs()).all()), (mode, scale)
                if scale in (0.125, -0.25):
                    assert torch.equal(got, x * scale)               # a power of two: exact


def test_functional_on_the_device_equals_its_cpu_path():
    x = DC.make_src(9, (6, 40, 40), 101)
    ops = DC.make_ops(12, DC.OPS, 102)
    index = DC.make_index("repeats", 12, 9, 103)
    xd = x.cuda()
    for mode in ("planes", "vector"):
        tables = DC.axis_tables(6) if mode == "vector" else None
        want = DC.restate(x, ops, index, tables)
        got = Fh.dihedral(xd, torch.tensor(ops, dtype=torch.int32, device="cuda"), index.cuda(), axis_mode=mode)
        DC.assert_same_bits(got, want, mode)
        DC.assert_same_bits(Fh.dihedral(xd, ops, index, axis_mode=mode), want, mode)            # host lists are moved over
        DC.assert_same_bits(Fh.dihedral(xd, tuple(ops), index.tolist(), axis_mode=mode), want, mode)
        DC.assert_same_bits(Fh.dihedral(x, ops, index, axis_mode=mode), want, mode)             # the torch-composed path
        DC.assert_same_bits(Fh.dihedral(xd.double(), ops, index, axis_mode=mode), want.double(), mode)
    with pytest.raises(_lib.TactileSRHipError):
        Fh.dihedral(xd, op_all=2, out=xd)                            # in place: refused before the launch
    y = x[:, 0].contiguous().cuda()                                  # (N, H, W)
    got = Fh.dihedral(y, op_all=5)
    assert got.shape == (9, 40, 40)
    DC.assert_same_bits(got, DC.restate(x[:, :1], [5] * 9)[:, 0])
    out = torch.full((9, 40, 40), NAN, device="cuda")
    assert Fh.dihedral(y, op_all=3, out=out).data_ptr() == out.data_ptr()
    DC.assert_same_bits(out, DC.restate(x[:, :1], [3] * 9)[:, 0])
    wide = DC.make_src(2, (1, 5, 7), 104).cuda()
    bad = Fh.dihedral(wide, [2, 1])                                  # a quarter turn of a non-square plane: refused per sample
    DC.assert_same_bits(bad[0], DC.restate(wide.cpu(), [2, 2])[0])
    assert bool(torch.isnan(bad[1]).all())
    with pytest.raises(_lib.TactileSRHipError):
        Fh.dihedral(wide, op_all=1)
    with pytest.raises(_lib.TactileSRHipError):
        Fh.dihedral(xd, op_all=0, accumulate=True)


# ------------------------------------------------------------------------------------------ self-ensemble, eval, loader
def _model(msrbs=2, seed=42):
    torch.manual_seed(seed)
    return tactilesr_amd.TactileSR(10, 1, 3, msrbs, 1).cuda()


def _taxels(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, 4, 4, generator=g) * 8


@pytest.mark.parametrize("mode", ["planes", "vector"])
@pytest.mark.parametrize("ops", ["dihedral", "rot90", (0, 5, 2)], ids=str)
def test_self_ensemble_is_the_mean_composed_op_by_op(ops, mode):
    m = _model().eval()
    LR = _taxels(3, 111)
    tables = DC.axis_tables(3) if mode == "vector" else None
    op_list = Fh.dihedral_ops(ops)
    n = len(op_list)
    mean = torch.zeros(3, 1, 40, 40, dtype=torch.float64)
    mag = torch.zeros_like(mean)
    with torch.no_grad():
        for op in op_list:
            y = m(DC.restate(LR, [op] * 3, None, tables).cuda()).cpu()
            back = DC.restate(y, [Fh.dihedral_inverse(op)] * 3).double() / n
            mean += back
            mag += back.abs()
    m.train()
    got = Fh.self_ensemble(m, LR.cuda(), ops, mode)
    assert m.training and not got.requires_grad
    err = (got.cpu().double() - mean).abs()
    bound = n * 2.0 ** -23 * mag
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float(mag.max()) > 0


def test_single_op_ensemble_is_the_model_bit_for_bit():
    m = _model().eval()
    LR = _taxels(3, 112).cuda()
    with torch.no_grad():
        want = m(LR)
    DC.assert_same_bits(Fh.self_ensemble(m, LR, (0,)), want)
    DC.assert_same_bits(Fh.self_ensemble(m, LR, (0,), "vector"), want)


def test_eval_func_without_self_ensemble_is_unchanged():
    m = _model(1)
    conf = TR.default_config()
    g = torch.Generator().manual_seed(113)
    LR, HR = _taxels(6, 114), torch.rand(6, 1, 100, 100, generator=g) * 100
    loader = DeviceSRLoader(LR, HR, 4)
    tot = [0.0, 0.0, 0.0]
    m.eval()
    with torch.no_grad():                                           # the loop as it stands in the parent commit
        for batch in loader:
            lr, hr = TR._prep(batch, conf, torch.device("cuda"))
            out = m(lr)
            ps, ss = Fh.psnr_ssim(out, hr, conf["sensorMaxVaule_factor"], reference_quirk=True)
            tot = [tot[0] + float(Fh.mse_loss(out, hr)), tot[1] + float(ss.mean()), tot[2] + float(ps.mean())]
    want = tuple(t / 2 for t in tot)
    assert TR.eval_func(m, loader, conf) == want
    assert TR.eval_func(m, loader, conf, self_ensemble=None) == want
    assert TR.eval_func(m, loader, conf, self_ensemble=(0,)) == want            # the one-op ensemble is the model
    four = TR.eval_func(m, loader, conf, windowed_ssim=True, self_ensemble=None)
    assert len(four) == 4 and four[:3] == want
    ens = TR.eval_func(m, loader, conf, self_ensemble="dihedral")
    assert len(ens) == 3 and all(v == v for v in ens) and ens != want


@pytest.mark.parametrize("augment,mode,axis", [("dihedral", "random", "planes"), ("rot90", "expand", "vector")])
def test_train_epoch_from_an_augmenting_loader(augment, mode, axis):
    conf = TR.default_config()
    g = torch.Generator().manual_seed(121)
    LR, HR = _taxels(6, 122), torch.rand(6, 1, 100, 100, generator=g) * 100
    loader = DeviceSRLoader(LR, HR, 4, shuffle=True, seed=7, augment=augment, augment_mode=mode, axis_mode=axis)
    n_ops = len(Fh.dihedral_ops(augment))
    assert len(loader) == (2 if mode == "random" else (6 * n_ops + 3) // 4)
    tables = DC.axis_tables(3) if axis == "vector" else None
    m = _model(1).train()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    pairs, losses = [], []
    for batch in loader:
        ops, idx = loader.last_ops.tolist(), loader.last_index.cpu()
        assert loader.last_ops.is_cuda and loader.last_ops.dtype == torch.int32 and loader.last_index.dtype == torch.int64
        DC.assert_same_bits(batch[0], DC.restate(LR, ops, idx, tables))
        DC.assert_same_bits(batch[1], DC.restate(HR, ops, idx))
        assert not batch[0].requires_grad and not batch[1].requires_grad
        pairs += list(zip(idx.tolist(), ops))
        losses.append(TR.train_one_iter(m, opt, batch, conf)["total_loss"])
    assert all(bool(torch.isfinite(v)) for v in losses)
    if mode == "expand":
        assert sorted(pairs) == [(s, o) for s in range(6) for o in range(n_ops)]
    else:
        assert sorted(p[0] for p in pairs) == list(range(6))
