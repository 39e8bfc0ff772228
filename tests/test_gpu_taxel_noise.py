"""GPU checks of the taxel sensor-noise launch (tsr_taxel_noise / _wgs / _dev / _bits, functional.taxel_noise, the noisy
DeviceSRLoader, eval_func's taxel_noise) against the numpy restatements of tests/_taxel_noise_cases.py: the generator and
the dropout mask bit for bit, the gain as the fp32 product, the noise within 1e-5 max(|v|, s) of fp64.  Every launch
writes into a NaN-prefilled output between NaN guard bands, reads x from a guarded buffer of its own, and runs twice:
the two runs must give the same bits."""
import numpy as np
import pytest
import torch

import _taxel_noise_cases as TN
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib, optim
from tactilesr_amd.data import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR

pytestmark = pytest.mark.gpu


def _lib_():
    return _lib.load()


def _fh_spec(sp):
    t = Fh.TaxelNoise(sigma_add=sp["sigma_add"], sigma_mul=sp["sigma_mul"], gain_jitter=sp["gain_jitter"],
                      drop_prob=sp["drop_thresh"] / TN.TWO24, drop_value=sp["drop_value"], axis_cnt=sp["axis_cnt"])
    assert t.drop_thresh == sp["drop_thresh"]
    return t


# ------------------------------------------------------------------------------------------------------------ generator
def _bits(B, blocks, tag, seed, offset, ids=None, id_base=0, expect=0):
    n = B * blocks * 4
    buf, out, start = TN.placed(n, 0, 64)
    idd = None if ids is None else torch.as_tensor(np.asarray(ids, dtype=np.int64)).cuda()
    a = dict(B=B, blocks=blocks, id_base=id_base, tag=tag, seed=seed, offset=offset)
    st = TN.call_bits_raw(_lib_(), a, stream=torch.cuda.current_stream().cuda_stream, out=out.data_ptr(),
                          ids=0 if idd is None else idd.data_ptr())
    assert st == expect
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:start]).all() and torch.isnan(buf[start + n:]).all()), "guard band written"
    return TN.bits(out).reshape(B, 4 * blocks)


def test_bits_equal_the_numpy_philox():
    """The known answer whose counter the launch can express (block 0 of id 0, offset 0, tag 0, seed 0) directly; the two
    others hold an id of 2^31 or more and the block 2^32 - 1, outside the launch's domain: they are checked on the numpy
    Philox (tests/test_taxel_noise_cpu.py), and the launch against that Philox on 25 200 blocks per tag and key."""
    counter, key, want = TN.KNOWN_ANSWERS[0]
    assert _bits(1, 1, 0, 0, 0)[0].tolist() == list(want)
    # the third known answer's key, offset and tag words, at an id the launch accepts
    seed, offset, tag = 0x299f31d0a4093822, 0x13198a2e, 0x03707344
    one = TN.philox((0, 0x05a308d3, offset, tag), (seed & 0xffffffff, seed >> 32))
    assert _bits(1, 1, tag, seed, offset, id_base=0x05a308d3)[0].tolist() == [int(v) for v in one]
    for t in (0, 1, 2):
        got = _bits(2100, 12, t, seed, offset, id_base=17)
        TN.assert_same_bits(got, TN.words(np.arange(17, 2117), 12, t, seed, offset), ("id_base", t))
        ids = TN.make_ids("high", 67, 5)                            # up to 2^31 - 1
        assert ids.max() == 2 ** 31 - 1
        TN.assert_same_bits(_bits(67, 3, t, 1, 0xffffffff, ids=ids), TN.words(ids, 3, t, 1, 0xffffffff), ("high ids", t))
    bad = _bits(3, 2, 0, 1, 1, ids=[5, 2 ** 31, -1])
    TN.assert_same_bits(bad[0], TN.words([5], 2, 0, 1, 1)[0])
    assert (bad[1:] == TN.NAN_BITS).all()
    TN.assert_same_bits(Fh.taxel_noise_bits(7, 5, 2, 9, 3, id_base=4).cpu().numpy().reshape(7, 20), TN.words(np.arange(4, 11), 5, 2, 9, 3))
    TN.assert_same_bits(Fh.taxel_noise_bits(7, 5, 2, 9, 3, id_base=4), Fh.taxel_noise_bits(7, 5, 2, 9, 3, id_base=4, device="cpu"))


# -------------------------------------------------------------------------------------------------------------- effects
@pytest.mark.parametrize("drop_value", [0.0, -1.5])
@pytest.mark.parametrize("thresh", [0, 1, 1 << 23, 1 << 24])
def test_dropout_mask_is_bit_exact(thresh, drop_value):
    B, shape = 2100, (6, 4, 4)
    x = TN.make_x(B, shape, 11)
    x.view(np.uint32)[::7, 1, 2, 3] = 0x7fc12345                     # NaN taxels: a dead one is replaced, an alive one keeps its payload
    sp = TN.spec(drop_thresh=thresh, drop_value=drop_value)
    got = TN.launch(_lib_(), x, sp, 4, 2, id_base=3)
    dead = TN.restate(x, sp, 4, 2, np.arange(3, B + 3))["dead"]
    TN.assert_same_bits(got, TN.apply_dropout(x, dead, drop_value))
    share = float(dead.mean())
    assert share == {0: 0.0, 1 << 24: 1.0}.get(thresh, share)
    if thresh == 1 << 23:
        assert TN.dead_z(dead, 0.5) <= 4.0
    TN.check(got, x, sp, 4, 2, None, id_base=3)


@pytest.mark.parametrize("gain_jitter", [0.25, 0.5, 0.1, -0.3])
def test_gain_alone(gain_jitter):
    for shape, a in (((21, 4, 4), 3), ((3, 5, 5), 3), ((6, 4, 4), 2)):
        x = TN.make_x(67, shape, 21)
        sp = TN.spec(gain_jitter=gain_jitter, axis_cnt=a)
        got = TN.launch(_lib_(), x, sp, 6, 1)
        TN.check(got, x, sp, 6, 1, None)                             # within 2^-24 of g x, and the fp32 product itself
        if gain_jitter in (0.25, 0.5):                               # gain_jitter (2 u - 1) is exact: plain fp32 gives the same g
            TN.assert_same_bits(got, TN.restate(x, sp, 6, 1, np.arange(67), np.float32)["v"], shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            frames = got.reshape(67, shape[0] // a, a, -1) / x.reshape(67, shape[0] // a, a, -1)
        # one gain per physical taxel, shared by the frames: two quotients of g x (1 + e) differ by 4 roundings of g < 2
        assert float(np.nanmax(np.abs(frames - frames[:, :1]))) <= 2.0 ** -21


CASES = [(s, a, B) for s, a, _ in TN.SHAPES for B in TN.BATCHES]


@pytest.mark.parametrize("shape,axis_cnt,B", CASES, ids=["%s-a%d-B%d" % ("x".join(map(str, s)), a, B) for s, a, B in CASES])
def test_every_shape_and_batch_against_fp64(shape, axis_cnt, B):
    x = TN.make_x(B, shape, 100 + B)
    specs = [sp for sp, _ in TN.SPECS] if axis_cnt == 3 else [TN.FULL2, TN.spec([0.02, 0.0], [0.0, 0.0], axis_cnt=2)]
    if B == 2100:
        specs = specs[:2]
    worst = 0.0
    for k, sp in enumerate(specs):
        got = TN.launch(_lib_(), x, sp, 7 + k, 3, id_base=5)
        worst = max(worst, TN.check(got, x, sp, 7 + k, 3, None, id_base=5))
    print("worst |kernel - fp64| / max(|v|, s):", shape, axis_cnt, B, worst)


@pytest.mark.parametrize("shape", [(3, 4, 4), (21, 4, 4), (3, 5, 5)], ids=str)
def test_bases_off_alignment_and_in_place(shape):
    x = TN.make_x(67, shape, 31)
    ids = TN.make_ids("perm", 67, 32)
    want = TN.launch(_lib_(), x, TN.FULL, 8, 2, ids=ids)
    TN.check(want, x, TN.FULL, 8, 2, ids)
    for xo in (0,) + TN.OFFSETS:
        for oo in (0,) + TN.OFFSETS:
            if xo or oo:
                TN.assert_same_bits(TN.launch(_lib_(), x, TN.FULL, 8, 2, ids=ids, x_off=xo, out_off=oo), want, (xo, oo))
        TN.assert_same_bits(TN.launch(_lib_(), x, TN.FULL, 8, 2, ids=ids, x_off=xo, inplace=True), want, ("in place", xo))


@pytest.mark.parametrize("shape", [(21, 4, 4), (3, 3, 7)], ids=str)
def test_ids_null_permuted_repeated_and_bad(shape):
    B = 67
    x = TN.make_x(B, shape, 41)
    base = TN.launch(_lib_(), x, TN.FULL, 2, 5, id_base=1000)
    TN.check(base, x, TN.FULL, 2, 5, None, id_base=1000)
    TN.assert_same_bits(TN.launch(_lib_(), x, TN.FULL, 2, 5, ids=np.arange(1000, 1000 + B)), base, "ids = id_base + b")
    for kind in ("perm", "repeats", "high"):
        ids = TN.make_ids(kind, B, 42)
        got = TN.launch(_lib_(), x, TN.FULL, 2, 5, ids=ids, id_base=77)         # id_base is not read next to ids
        TN.check(got, x, TN.FULL, 2, 5, ids)
    # a repeated id: identical noise.  The same sample under the same id twice gives the same bits.
    x2 = x.copy()
    x2[1] = x2[0]
    ids = TN.make_ids("perm", B, 43)
    ids[1] = ids[0]
    got = TN.launch(_lib_(), x2, TN.FULL, 2, 5, ids=ids)
    TN.assert_same_bits(got[0], got[1])
    # bad ids: all-NaN samples, bit-identical neighbours
    clean = TN.launch(_lib_(), x, TN.FULL, 2, 5, ids=TN.make_ids("perm", B, 44))
    ids = TN.make_ids("perm", B, 44)
    ids[[0, 5, 66]] = [-1, 2 ** 31, -2 ** 40]
    got = TN.launch(_lib_(), x, TN.FULL, 2, 5, ids=ids)
    TN.check(got, x, TN.FULL, 2, 5, ids)
    keep = np.setdiff1d(np.arange(B), [0, 5, 66])
    TN.assert_same_bits(got[keep], clean[keep])
    assert (TN.bits(got[[0, 5, 66]]) == TN.NAN_BITS).all()
    got = TN.launch(_lib_(), x, TN.FULL, 2, 5, id_base=2 ** 31 - 3)              # ids run past 2^31 - 1 inside the batch
    TN.check(got, x, TN.FULL, 2, 5, None, id_base=2 ** 31 - 3)
    assert np.isnan(got[3:]).all() and not np.isnan(got[:3]).all()


@pytest.mark.parametrize("max_wgs", [w for w, _ in TN.WALKS])
@pytest.mark.parametrize("shape,B", [((21, 4, 4), 67), ((3, 5, 5), 67), ((3, 4, 4), 2100)], ids=str)
def test_capped_grids_walk_to_the_same_bits(shape, B, max_wgs):
    """5628, 1273 and 25 200 work items over 1 and 3 workgroups of 256, a NaN sample in the middle of the walk."""
    x = TN.make_x(B, shape, 51)
    ids = TN.make_ids("perm", B, 52)
    ids[B // 2] = -7
    want = TN.launch(_lib_(), x, TN.FULL, 3, 9, ids=ids)
    TN.assert_same_bits(TN.launch(_lib_(), x, TN.FULL, 3, 9, ids=ids, max_wgs=max_wgs), want)
    TN.assert_same_bits(TN.launch(_lib_(), x, TN.FULL, 3, 9, ids=ids, max_wgs=1 << 20), want)
    TN.assert_same_bits(TN.launch(_lib_(), x, TN.FULL, 3, 9, ids=ids, max_wgs=max_wgs, inplace=True), want)


def test_dev_form_equals_the_scalar_form():
    for shape, a, sp in (((21, 4, 4), 3, TN.FULL), ((3, 5, 5), 3, TN.FULL), ((6, 4, 4), 2, TN.FULL2)):
        x = TN.make_x(67, shape, 61)
        for seed, offset in ((0, 0), (0xfedcba9876543210, 0xffffffff), (5, 7)):
            want = TN.launch(_lib_(), x, sp, seed, offset, id_base=9)
            TN.assert_same_bits(TN.launch(_lib_(), x, sp, id_base=9, rng=(seed, offset)), want, (shape, seed))
            TN.assert_same_bits(TN.launch(_lib_(), x, sp, id_base=9, rng=(seed, offset), inplace=True, x_off=1), want)


def test_graph_capture_draws_fresh_noise_per_replay():
    x = torch.from_numpy(TN.make_x(67, (21, 4, 4), 71)).cuda()
    sp = _fh_spec(TN.FULL)
    ids = torch.from_numpy(TN.make_ids("perm", 67, 72)).cuda()
    rng = Fh.taxel_noise_rng(11, 0)
    out = torch.full_like(x, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Fh.taxel_noise(x, sp, ids=ids, out=out, rng=rng)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Fh.taxel_noise(x, sp, ids=ids, out=out, rng=rng)
    seen = []
    for offset in (1, 2, 3):
        rng[2] = offset                                             # the host rewrites the offset word
        graph.replay()
        seen.append(out.clone())
    torch.cuda.synchronize()
    for offset, got in zip((1, 2, 3), seen):
        TN.assert_same_bits(got, Fh.taxel_noise(x, sp, 11, offset, ids=ids), offset)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    TN.check(seen[2].cpu().numpy(), x.cpu().numpy(), TN.FULL, 11, 3, ids.cpu().numpy())


@pytest.mark.parametrize("shape", [(21, 4, 4), (3, 5, 5)], ids=str)
def test_nonfinite_elements_stay_in_their_own_element(shape):
    x = TN.make_x(67, shape, 81)
    flat = x.view(np.uint32).reshape(-1)
    specials = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000], dtype=np.uint32)
    where = torch.randperm(flat.size, generator=torch.Generator().manual_seed(82))[:6 * len(specials)].numpy()
    flat[where] = np.tile(specials, 6)
    for sp, _ in TN.SPECS:
        got = TN.launch(_lib_(), x, sp, 1, 1)
        TN.check(got, x, sp, 1, 1, None)
        if sp["drop_thresh"] == 0:
            assert np.array_equal(np.isfinite(got), np.isfinite(x))
    TN.assert_same_bits(TN.launch(_lib_(), x, TN.NEUTRAL, 1, 1), x, "all neutral: the identity, payloads and -0 included")
    TN.assert_same_bits(TN.launch(_lib_(), x, TN.NEUTRAL, 1, 1, x_off=1, out_off=2), x)
    TN.assert_same_bits(TN.launch(_lib_(), x, TN.spec(drop_thresh=1 << 24, drop_value=0.25), 1, 1), np.full_like(x, 0.25))


def test_statistics_of_the_kernels_own_output():
    c = TN.STAT_CASE
    B, shape = c["B"], c["shape"]
    zeros = np.zeros((B,) + shape, dtype=np.float32)
    n1 = TN.launch(_lib_(), zeros, TN.spec(sigma_add=1.0), c["seed"], c["offset"])       # v = 0, s = 1: the normals themselves
    s = TN.stats(n1)
    print("kernel normals: mean, var, KS (scaled):", s)
    assert all(v <= lim for v, lim in zip(s, TN.STAT_LIMITS)), s
    assert float(np.abs(n1).max()) <= 5.77
    n64 = TN.restate(zeros, TN.spec(sigma_add=1.0), c["seed"], c["offset"], np.arange(B))["n"]
    print("kernel normals: worst |n - n64| =", float(np.abs(n1 - n64).max()))
    n2 = TN.launch(_lib_(), zeros, TN.spec(sigma_add=1.0), c["seed"], c["offset"] + 1)
    assert TN.corr_scaled(n1, n2) <= 4.0
    ones = np.ones_like(zeros)
    g = TN.launch(_lib_(), ones, TN.spec(gain_jitter=0.5), c["seed"], c["offset"])       # 1 + (2 u - 1) / 2: the gain uniforms
    assert TN.corr_scaled(n1, g) <= 4.0                              # between tags 0 and 1
    assert abs(float(g.astype(np.float64).mean()) - 1.0) * np.sqrt(12 * g.size) <= 4.0   # uniform on [1/2, 3/2): variance 1/12
    d = TN.launch(_lib_(), ones, TN.spec(drop_prob=0.1), c["seed"], c["offset"])
    dead = d[:, 0] == 0.0
    assert np.array_equal(d == 0.0, np.broadcast_to(dead[:, None], d.shape))              # every channel of a dead taxel
    z = TN.dead_z(dead, TN.spec(drop_prob=0.1)["drop_thresh"] / TN.TWO24)
    print("kernel dead share z:", z)
    assert z <= 4.0
    assert TN.corr_scaled(n1[:, 0], dead.astype(np.float64)) <= 4.0                       # between tags 0 and 2


def test_functional_on_the_device():
    x = TN.make_x(67, (21, 4, 4), 91)
    xd = torch.from_numpy(x).cuda()
    sp = _fh_spec(TN.FULL)
    ids = TN.make_ids("perm", 67, 92)
    want = TN.launch(_lib_(), x, TN.FULL, 13, 4, ids=ids)
    got = Fh.taxel_noise(xd, sp, 13, 4, ids=torch.from_numpy(ids).cuda())
    TN.assert_same_bits(got, want)
    assert not got.requires_grad and got.data_ptr() != xd.data_ptr()
    TN.assert_same_bits(Fh.taxel_noise(xd, TN_dict(sp), 13, 4, ids=ids.tolist()), want)   # a dict spec, host ids
    y = xd.clone()
    assert Fh.taxel_noise(y, sp, 13, 4, ids=ids, out=y) is y
    TN.assert_same_bits(y, want)
    TN.assert_same_bits(Fh.taxel_noise(xd, sp, ids=ids, rng=Fh.taxel_noise_rng(13, 4)), want)
    TN.assert_same_bits(Fh.taxel_noise(xd[:, :6][:, ::1], sp, 13, 4, ids=ids), TN.launch(_lib_(), x[:, :6].copy(), TN.FULL, 13, 4, ids=ids))
    TN.assert_same_bits(Fh.taxel_noise(xd, None), x)
    cpu = Fh.taxel_noise(torch.from_numpy(x), sp, 13, 4, ids=ids).numpy()            # the numpy path: same stream, a few ulp
    TN.check(cpu, x, TN.FULL, 13, 4, ids, bar=TN.F32_BAR)
    assert np.array_equal(cpu == np.float32(-1.5), want == np.float32(-1.5))
    flat, n66 = xd.view(-1), 66 * 336
    with pytest.raises(_lib.TactileSRHipError):                      # a partial overlap: refused before the launch
        Fh.taxel_noise(flat[:n66].view(66, 21, 4, 4), sp, out=flat[4:4 + n66].view(66, 21, 4, 4))
    with pytest.raises(_lib.TactileSRHipError):
        Fh.taxel_noise(xd, sp, rng=torch.zeros(4, dtype=torch.int32))               # rng on another device


def TN_dict(t):
    return dict(sigma_add=t.sigma_add, sigma_mul=t.sigma_mul, gain_jitter=t.gain_jitter, drop_prob=t.drop_prob,
                drop_value=t.drop_value, axis_cnt=t.axis_cnt)


# -------------------------------------------------------------------------------------------------- loader, train, eval
def _model(msrbs=1, seed=42, **kw):
    torch.manual_seed(seed)
    return tactilesr_amd.TactileSR(10, 1, 3, msrbs, 1, **kw).cuda()


def _taxels(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, 4, 4, generator=g) * 8


def test_train_epoch_from_a_noisy_augmenting_loader():
    conf = TR.default_config()
    g = torch.Generator().manual_seed(121)
    LR, HR = _taxels(6, 122), torch.rand(6, 1, 100, 100, generator=g) * 100
    kw = dict(shuffle=True, seed=7, augment="dihedral", augment_mode="random")
    sp = Fh.TaxelNoise(sigma_add=0.05, sigma_mul=0.05, gain_jitter=0.1, drop_prob=0.1)
    clean, noisy = DeviceSRLoader(LR, HR, 4, **kw), DeviceSRLoader(LR, HR, 4, taxel_noise=sp, noise_seed=3, **kw)
    m = _model().train()
    opt = optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    it = iter(clean)
    for batch in noisy:
        l0, h0 = next(it)
        assert torch.equal(noisy.last_index, clean.last_index) and torch.equal(noisy.last_ops, clean.last_ops)
        TN.assert_same_bits(batch[1], h0, "HR")
        assert not torch.equal(batch[0], l0) and not batch[0].requires_grad
        TN.assert_same_bits(batch[0], Fh.taxel_noise(l0, sp, 3, 1, ids=noisy.last_index))
        losses.append(TR.train_one_iter(m, opt, batch, conf)["total_loss"])
    assert len(losses) == 2 and all(bool(torch.isfinite(v)) for v in losses)
    TN.assert_same_bits(noisy.LR, LR)


def test_eval_func_on_degraded_taxels_does_not_depend_on_the_batch_size():
    """24 samples at test batch sizes 8 and 3: the model meets bit-identical taxels, sample for sample.  With the fp32 eval
    arithmetic a sample's output does not depend on its batch, so the scores differ only by the order of fp32 / fp64
    sums over equal-sized batches: within 1e-5 relative."""
    m = _model(conv_impl="f32")
    conf = TR.default_config()
    g = torch.Generator().manual_seed(131)
    LR, HR = _taxels(24, 132), torch.rand(24, 1, 100, 100, generator=g) * 100
    sp = Fh.TaxelNoise(sigma_add=0.05, sigma_mul=0.05, gain_jitter=0.1, drop_prob=0.1)
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append(args[0].clone()))
    res = {}
    for bs in (8, 3):
        seen.clear()
        res[bs] = TR.eval_func(m, DeviceSRLoader(LR, HR, bs), conf, taxel_noise=sp, noise_seed=5)
        res[bs, "x"] = torch.cat(seen)
    hook.remove()
    TN.assert_same_bits(res[8, "x"], res[3, "x"])
    TN.assert_same_bits(res[8, "x"], Fh.taxel_noise(LR.cuda(), sp, 5, 0))
    print("eval at batch sizes 8 and 3:", res[8], res[3])
    assert all(abs(a - b) <= 1e-5 * abs(a) for a, b in zip(res[8], res[3])), (res[8], res[3])
    clean = TR.eval_func(m, DeviceSRLoader(LR, HR, 8), conf)
    assert clean == TR.eval_func(m, DeviceSRLoader(LR, HR, 8), conf, taxel_noise=None, noise_seed=5) and clean != res[8]
    assert TR.eval_func(m, DeviceSRLoader(LR, HR, 8), conf, taxel_noise=sp, noise_seed=5) == res[8]
    ens = TR.eval_func(m, DeviceSRLoader(LR, HR, 8), conf, self_ensemble="rot90", taxel_noise=sp, noise_seed=5)
    assert len(ens) == 3 and all(v == v for v in ens)


# ------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("label,over", TN.REFUSALS, ids=[r[0] for r in TN.REFUSALS])
def test_refusals_leave_the_output_untouched(label, over):
    a = dict(TN.BASE_ARGS, **over)
    n = 4 * 48
    buf = torch.full((2 * n + 64,), float("nan"), device="cuda")
    x, out = buf[:n], buf[n + 32:2 * n + 32]
    x.copy_(torch.from_numpy(TN.make_x(4, (3, 4, 4), 141)).reshape(-1))
    before = buf.clone()
    ids = torch.arange(4, device="cuda")
    rng = Fh.taxel_noise_rng(1, 1)
    ptrs = dict(ids=ids.data_ptr())
    if a["x"]:
        ptrs["x"] = x.data_ptr()
    if a["out"]:
        ptrs["out"] = out.data_ptr()
    if a.get("rng"):
        ptrs["rng"] = rng.data_ptr()
    if abs(a["B"] * a["C"] * a["H"] * a["W"]) > n or abs(a.get("overlap", 0)) > 4 * n:
        ptrs = {}                                                   # a shape the buffers do not hold: fake addresses only
    st = TN.call_raw(_lib_(), a, stream=torch.cuda.current_stream().cuda_stream, **ptrs)
    torch.cuda.synchronize()
    assert st == 1, label
    TN.assert_same_bits(buf, before, label)
