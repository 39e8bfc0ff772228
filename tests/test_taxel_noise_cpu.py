"""CPU checks of the taxel sensor-noise augmentation: the Philox known answers, the fp32 restatements against fp64, the
statistics of the stream, the spec, the symbols and their refusals, the loader / tpsf_loader / eval_func plumbing on
device="cpu" (functional.taxel_noise's numpy path).  No GPU: refusals return before any device call."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _taxel_noise_cases as TN
import tactilesr_amd.data as D
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib
from tactilesr_amd.data import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = _lib.TactileSRHipError


def _fh_spec(sp):
    """The functional.TaxelNoise of a cases dict whose drop_thresh came from a drop_prob."""
    t = Fh.TaxelNoise(sigma_add=sp["sigma_add"], sigma_mul=sp["sigma_mul"], gain_jitter=sp["gain_jitter"],
                      drop_prob=sp["drop_thresh"] / TN.TWO24, drop_value=sp["drop_value"], axis_cnt=sp["axis_cnt"])
    assert t.drop_thresh == sp["drop_thresh"]
    return t


# ------------------------------------------------------------------------------------------------------------ generator
@pytest.mark.parametrize("counter,key,want", TN.KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in TN.philox(counter, key)) == want
    assert tuple(int(w) for w in Fh._philox_np(*counter, *key)) == want          # the product's own restatement


def test_words_layout_and_the_functional_stream():
    ids = np.array([0, 5, 2 ** 31 - 1], dtype=np.int64)
    seed, offset = 0x299f31d0a4093822, 0x13198a2e
    for tag in (0, 1, 2):
        w = TN.words(ids, 6, tag, seed, offset)
        assert w.shape == (3, 24) and w.dtype == np.uint32
        one = TN.philox((4, 5, offset, tag), (seed & 0xffffffff, seed >> 32))   # block 4 of sample id 5
        assert [int(v) for v in one] == w[1, 16:20].tolist()
        got = Fh.taxel_noise_bits(3, 6, tag, seed, offset, ids=ids, device="cpu")
        assert got.dtype == torch.int32 and got.shape == (3, 6, 4)
        TN.assert_same_bits(got.numpy().reshape(3, 24), w, tag)
    base = Fh.taxel_noise_bits(3, 2, 0, 7, 1, id_base=11, device="cpu")
    TN.assert_same_bits(base.numpy().reshape(3, 8), TN.words(np.arange(11, 14), 2, 0, 7, 1))
    bad = Fh.taxel_noise_bits(2, 2, 0, ids=[-1, 2 ** 31], device="cpu")
    assert (TN.bits(bad) == TN.NAN_BITS).all()
    for kw in (dict(B=0), dict(blocks=0), dict(tag=-1), dict(offset=-1), dict(offset=2 ** 32), dict(ids=[1])):
        with pytest.raises(ERR):
            Fh.taxel_noise_bits(**dict(dict(B=2, blocks=2, tag=0, device="cpu"), **kw))


# ----------------------------------------------------------------------------------------------- restatements, statistics
def test_fp32_restatements_stay_within_the_bar_of_fp64():
    """Both fp32 restatements -- the plain numpy one of the cases file and functional.taxel_noise's CPU path -- against the
    fp64 one: |y32 - y64| <= 2e-6 max(|v|, s) per element, the normals within 1.6e-6 absolute."""
    B, shape = 4096, (3, 4, 4)
    x = TN.make_x(B, shape, 11)
    sp = TN.spec(0.02, 0.05)
    ids = np.arange(B)
    r64, r32 = TN.restate(x, sp, 0, 1, ids), TN.restate(x, sp, 0, 1, ids, np.float32)
    assert r32["y"].dtype == np.float32
    dn = float(np.abs(r32["n"] - r64["n"]).max())
    print("normals: worst |n32 - n64| =", dn)
    assert dn <= 1.6e-6
    assert float(np.abs(r64["n"]).max()) <= 5.77
    scale = np.maximum(np.abs(r64["v"]), r64["s"])
    for name, y32 in (("cases", r32["y"]), ("functional", Fh.taxel_noise(torch.from_numpy(x), _fh_spec(sp), 0, 1).numpy())):
        worst = float((np.abs(y32 - r64["y"]) / scale).max())
        print(name, "worst |y32 - y64| / max(|v|, s) =", worst)
        assert worst <= TN.F32_BAR, (name, worst)
    # the whole contract through the checker, at its own (wider) bar, on every spec and the scalar-path shapes
    for sp, _ in TN.SPECS:
        for shape in ((3, 4, 4), (21, 4, 4), (3, 5, 5)):
            x = TN.make_x(67, shape, 12)
            got = Fh.taxel_noise(torch.from_numpy(x), _fh_spec(sp), 3, 2, id_base=100).numpy()
            TN.check(got, x, sp, 3, 2, None, id_base=100, bar=TN.F32_BAR)


def test_statistics_of_the_stream():
    c = TN.STAT_CASE
    B, (C, H, W) = c["B"], c["shape"]
    nb = C * H * W // 4
    ids = np.arange(B)
    n1 = TN.normals(TN.words(ids, nb, 0, c["seed"], c["offset"]), np.float64)
    assert n1.size == 196608
    s = TN.stats(n1)
    print("mean, var, KS (scaled):", s)
    assert all(v <= lim for v, lim in zip(s, TN.STAT_LIMITS)), s
    # the product's path gives these normals: zeros in, sigma_add = 1
    y = Fh.taxel_noise(torch.zeros(B, C, H, W), Fh.TaxelNoise(sigma_add=1.0), c["seed"], c["offset"]).numpy()
    assert float(np.abs(y.reshape(B, -1) - n1).max()) <= 1.6e-6
    n2 = TN.normals(TN.words(ids, nb, 0, c["seed"], c["offset"] + 1), np.float64)
    assert TN.corr_scaled(n1, n2) <= 4.0
    # between tags: the same counters under tag 1 and tag 2 against tag 0, as uniforms
    u = [(TN.words(ids, nb, t, c["seed"], c["offset"]) >> 8).astype(np.float64) for t in (0, 1, 2)]
    assert TN.corr_scaled(u[0], u[1]) <= 4.0 and TN.corr_scaled(u[0], u[2]) <= 4.0 and TN.corr_scaled(u[1], u[2]) <= 4.0
    # consecutive ids and consecutive seeds
    n3 = TN.normals(TN.words(ids + 1, nb, 0, c["seed"] + 1, c["offset"]), np.float64)
    assert TN.corr_scaled(n1, n3) <= 4.0
    sp = TN.spec(drop_prob=0.1)
    dead = TN.restate(np.zeros((B, C, H, W), np.float32), sp, c["seed"], c["offset"], ids)["dead"]
    z = TN.dead_z(dead, sp["drop_thresh"] / TN.TWO24)
    print("dead share z:", z, dead.mean())
    assert z <= 4.0
    # gain uniforms: mean 1/2, variance 1/12
    g = (TN.words(ids, 12, 1, c["seed"], c["offset"]) >> 8).astype(np.float64) * 2.0 ** -24
    assert abs(g.mean() - 0.5) * np.sqrt(12 * g.size) <= 4.0


def test_noise_is_a_function_of_seed_offset_id_only():
    LR, HR = torch.from_numpy(TN.make_x(23, (6, 4, 4), 21)), torch.zeros(23, 1, 8, 8)
    sp = _fh_spec(TN.FULL)
    whole = Fh.taxel_noise(LR, sp, 9, 1).numpy()
    # the launch: any subset, any order, repeated ids
    ids = np.array([22, 3, 3, 0, 17], dtype=np.int64)
    part = Fh.taxel_noise(LR[ids], sp, 9, 1, ids=ids).numpy()
    TN.assert_same_bits(part, whole[ids])
    TN.assert_same_bits(part[1], part[2])
    TN.assert_same_bits(Fh.taxel_noise(LR[5:9], sp, 9, 1, id_base=5).numpy(), whole[5:9])
    assert not np.array_equal(Fh.taxel_noise(LR, sp, 9, 2).numpy(), whole)              # another offset
    assert not np.array_equal(Fh.taxel_noise(LR, sp, 10, 1).numpy(), whole)             # another seed
    # through the loader: batch size, shuffling and position do not matter
    for bs, shuffle, seed in ((4, False, 9), (7, True, 9), (23, True, 9), (5, True, 9)):
        ld = DeviceSRLoader(LR, HR, bs, shuffle=shuffle, seed=seed, device="cpu", taxel_noise=sp)
        g = torch.Generator().manual_seed(seed)
        order = torch.randperm(23, generator=g) if shuffle else torch.arange(23)
        got = torch.cat([b[0] for b in ld]).numpy()
        TN.assert_same_bits(got, whole[order.numpy()], (bs, shuffle))
    other = DeviceSRLoader(LR, HR, 4, seed=1, noise_seed=9, device="cpu", taxel_noise=sp)
    TN.assert_same_bits(torch.cat([b[0] for b in other]).numpy(), whole, "noise_seed")


def test_all_neutral_is_the_identity_bit_for_bit():
    x = TN.make_x(5, (3, 4, 4), 31)
    xb = x.view(np.uint32)
    xb[0, 0, 0, :4] = [0x7fc12345, 0xffc00001, 0x7f800001, 0x80000000]                 # NaN payloads, a signalling NaN, -0
    xb[1, 1, 1, :3] = [0x7f800000, 0xff800000, 0x00000001]                             # +-Inf, a subnormal
    for sp in (Fh.TaxelNoise(), None, {}, dict(sigma_add=[0, 0, 0], drop_prob=1e-9), Fh.TaxelNoise(axis_cnt=1)):
        got = Fh.taxel_noise(torch.from_numpy(x), sp, 123, 4)
        TN.assert_same_bits(got.numpy(), x)
        assert got.data_ptr() != torch.from_numpy(x).data_ptr()
    assert Fh.TaxelNoise().is_identity and Fh.TaxelNoise(drop_prob=1e-9).is_identity
    for kw in (dict(sigma_add=0.1), dict(sigma_mul=[0, 0, 1e-3]), dict(gain_jitter=-0.1), dict(drop_prob=1e-7)):
        assert not Fh.TaxelNoise(**kw).is_identity, kw
    # dropout replaces a NaN; a NaN stays in its own element under noise
    got = Fh.taxel_noise(torch.from_numpy(x), dict(drop_prob=1.0, drop_value=-1.5)).numpy()
    assert (got == -1.5).all()
    got = Fh.taxel_noise(torch.from_numpy(x), dict(sigma_add=0.1, sigma_mul=0.1, gain_jitter=0.1)).numpy()
    assert np.array_equal(np.isfinite(got), np.isfinite(x))
    # a bad id: that sample all-NaN, the neighbours as before
    sp = _fh_spec(TN.FULL)
    clean = Fh.taxel_noise(torch.from_numpy(x), sp, 1, 1, ids=[4, 3, 2, 1, 0]).numpy()
    got = Fh.taxel_noise(torch.from_numpy(x), sp, 1, 1, ids=[4, -1, 2, 2 ** 31, 0]).numpy()
    assert (TN.bits(got[[1, 3]]) == TN.NAN_BITS).all()
    TN.assert_same_bits(got[[0, 2, 4]], clean[[0, 2, 4]])


def test_in_place_and_out_on_the_cpu_path():
    x = torch.from_numpy(TN.make_x(6, (3, 4, 4), 41))
    sp = _fh_spec(TN.FULL)
    want = Fh.taxel_noise(x, sp, 2, 3)
    out = torch.full_like(x, float("nan"))
    assert Fh.taxel_noise(x, sp, 2, 3, out=out) is out
    TN.assert_same_bits(out, want)
    y = x.clone()
    assert Fh.taxel_noise(y, sp, 2, 3, out=y) is y
    TN.assert_same_bits(y, want)
    rng = Fh.taxel_noise_rng(2, 3, device="cpu")
    assert rng.dtype == torch.int32 and rng.tolist() == [2, 0, 3, 0]
    TN.assert_same_bits(Fh.taxel_noise(x, sp, rng=rng), want)
    big = Fh.taxel_noise_rng(0xfedcba9876543210, 0xffffffff, device="cpu")
    TN.assert_same_bits(Fh.taxel_noise(x, sp, rng=big), Fh.taxel_noise(x, sp, 0xfedcba9876543210, 0xffffffff))
    assert not want.requires_grad and not Fh.taxel_noise(x.clone().requires_grad_(), sp).requires_grad
    flat = torch.zeros(6 * 48 + 8)
    with pytest.raises(ERR):
        Fh.taxel_noise(flat[:288].view(6, 3, 4, 4), sp, out=flat[4:292].view(6, 3, 4, 4))          # a partial overlap
    for bad in (dict(x=x[0]), dict(x=x.double()), dict(out=torch.zeros(5, 3, 4, 4)), dict(ids=[0, 1]), dict(offset=-1),
                dict(offset=2 ** 32), dict(rng=torch.zeros(3, dtype=torch.int32)), dict(rng=torch.zeros(4)),
                dict(spec=dict(axis_cnt=2)), dict(spec="gauss")):
        kw = dict(dict(x=x, spec=sp), **bad)
        with pytest.raises(ERR):
            Fh.taxel_noise(kw.pop("x"), kw.pop("spec"), **kw)


# ------------------------------------------------------------------------------------------------------------------ spec
def test_spec_validation():
    t = Fh.TaxelNoise(0.02, [0.05, 0.05, 0.1], 0.1, 0.1, -1.5)
    assert t.sigma_add == (np.float32(0.02),) * 3 and len(t.sigma_mul) == 3 and t.axis_cnt == 3
    assert t.drop_thresh == 1677722 == TN.FULL["drop_thresh"] and not t.is_identity
    assert Fh.TaxelNoise(drop_prob=1.0).drop_thresh == 1 << 24 and Fh.TaxelNoise(drop_prob=0.5).drop_thresh == 1 << 23
    assert Fh.TaxelNoise(drop_prob=2.0 ** -24).drop_thresh == 1
    with pytest.raises(Exception):
        t.gain_jitter = 0.2                                             # frozen
    assert hash(t) == hash(Fh.TaxelNoise(0.02, [0.05, 0.05, 0.1], 0.1, 0.1, -1.5))
    assert Fh.taxel_noise_spec(t) is t and Fh.taxel_noise_spec(None) is None
    assert Fh.taxel_noise_spec(dict(sigma_add=0.02, axis_cnt=2)) == Fh.TaxelNoise(sigma_add=0.02, axis_cnt=2)
    inf, nan = float("inf"), float("nan")
    for kw in (dict(sigma_add=-0.1), dict(sigma_mul=[0.1, -0.1, 0.1]), dict(sigma_add=nan), dict(sigma_mul=inf),
               dict(sigma_add=[0.1, 0.1]), dict(sigma_add=[0.1] * 4), dict(sigma_add="x"), dict(gain_jitter=nan),
               dict(gain_jitter=inf), dict(drop_value=nan), dict(drop_value=-inf), dict(drop_prob=-0.1), dict(drop_prob=1.5),
               dict(drop_prob=nan), dict(axis_cnt=0), dict(axis_cnt=5), dict(axis_cnt=2.0), dict(axis_cnt=True),
               dict(gain_jitter="a")):
        with pytest.raises(ERR):
            Fh.TaxelNoise(**kw)
    for bad in (dict(sigma=0.1), "noise", 0.1, [0.1]):
        with pytest.raises(ERR):
            Fh.taxel_noise_spec(bad)
    sig = inspect.signature(Fh.taxel_noise).parameters
    assert [sig[k].default for k in ("seed", "offset", "ids", "id_base", "out", "rng")] == [0, 0, None, 0, None, None]
    for fn in (Fh.taxel_noise, DeviceSRLoader):
        assert "autograd" in fn.__doc__


# --------------------------------------------------------------------------------------------------------------- symbols
NAMES = ("tsr_taxel_noise", "tsr_taxel_noise_wgs", "tsr_taxel_noise_dev", "tsr_taxel_noise_bits")


def test_symbols_declared_bound_and_exported_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24
    for name, nargs in zip(NAMES, (17, 18, 16, 9)):
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % name, header, re.M)
        assert decl, f"{name} is not declared in include/tactilesr_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name), name
    para = header[header.index("Taxel sensor-noise augmentation on the device"):header.index("int tsr_taxel_noise(")]
    for text in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(block, id, offset, tag)", "(seed_lo, seed_hi)",
                 "g = fmaf(gain_jitter, 2 u - 1, 1)", "u1 = (2 (ra >> 9) + 1) 2^-24", "R = sqrtf(-2 logf(u1))",
                 "cospif(2 u2)", "sinpif(2 u2)", "y = fmaf(s, n, v)", "(r >> 8) < drop_thresh", "Refusals"):
        assert text in para, text
    cap = re.search(r"^#define\s+TSR_TAXEL_NOISE_MAX_WGS\s+\(1 << (\d+)\)", header, re.M)
    assert cap and int(cap.group(1)) == 20
    declared = set(re.findall(r"^(?:int|long long)\s+(\w+)\s*\(", header, re.M))
    assert declared == set(_lib.SIGNATURES)
    src = open(os.path.join(REPO, "tactilesr_amd", "csrc", "taxel_noise.hip")).read()
    assert "getenv" not in src and "asm" not in src and "__shared__" not in src
    assert "atomic" not in src.replace("no atomics", "") and "__logf" not in src and "__cosf" not in src and "__sinf" not in src


@pytest.mark.parametrize("label,over", TN.REFUSALS, ids=[r[0] for r in TN.REFUSALS])
def test_refusals_need_no_device(label, over):
    """Status 1 before any device call: the pointers are small fake addresses nothing may dereference."""
    assert TN.call_raw(_lib.load(), dict(TN.BASE_ARGS, **over)) == 1, label


@pytest.mark.parametrize("label,over", TN.BITS_REFUSALS, ids=[r[0] for r in TN.BITS_REFUSALS])
def test_bits_refusals_need_no_device(label, over):
    assert TN.call_bits_raw(_lib.load(), dict(TN.BITS_BASE, **over)) == 1, label


def test_refusal_table_covers_the_contract():
    keys = {k for _, over in TN.REFUSALS for k in over}
    assert keys >= {"x", "out", "B", "C", "H", "W", "axis_cnt", "sigma_add", "sigma_mul", "gain_jitter", "drop_value",
                    "drop_thresh", "overlap", "max_wgs", "rng"}
    assert all(why for _, why in TN.SPECS) and all(why for _, _, why in TN.SHAPES)
    assert {s[1] * s[2] % 4 == 0 for s, _, _ in TN.SHAPES} == {True, False}             # both paths


# ------------------------------------------------------------------------------------------- loader, tpsf_loader, eval
def _set(n=10, seed=51):
    return torch.from_numpy(TN.make_x(n, (3, 4, 4), seed)), torch.from_numpy(TN.make_x(n, (1, 12, 12), seed + 1))[:, 0]


def test_loader_without_noise_is_todays_loader():
    LR, HR = _set()
    for shuffle in (False, True):
        a = DeviceSRLoader(LR, HR, 4, shuffle=shuffle, seed=5, device="cpu", taxel_noise=None, noise_seed=77)
        assert a._noise is None
        g = torch.Generator().manual_seed(5)                            # the loader as it was: one randperm per epoch
        for _ in range(2):
            order = torch.randperm(10, generator=g) if shuffle else torch.arange(10)
            got = list(a)
            assert len(got) == len(a) == 3
            for i, (l, h) in enumerate(got):
                idx = order[4 * i:4 * i + 4]
                TN.assert_same_bits(l, LR[idx]), TN.assert_same_bits(h, HR[idx])
        assert torch.equal(a._gen.get_state(), g.get_state())
    plain = DeviceSRLoader(LR, HR, 4, device="cpu")
    assert next(iter(plain))[0].data_ptr() == plain.LR.data_ptr()       # still a view of the set


@pytest.mark.parametrize("augment,mode", [(None, "random"), ("dihedral", "random"), ("rot90", "expand")])
def test_loader_noise_leaves_index_ops_generator_and_HR_alone(augment, mode):
    LR, HR = _set(11, 61)
    HR = HR.unsqueeze(1)
    sp = _fh_spec(TN.FULL)
    kw = dict(shuffle=True, seed=3, device="cpu", augment=augment, augment_mode=mode)
    off, on = DeviceSRLoader(LR, HR, 4, **kw), DeviceSRLoader(LR, HR, 4, taxel_noise=sp, noise_seed=8, **kw)
    assert len(off) == len(on)
    for epoch in (1, 2):
        n_ops = len(on._ops) if augment else 1
        g = torch.Generator().manual_seed(3)
        for _ in range(epoch):
            order = torch.randperm(len(LR) * (n_ops if mode == "expand" else 1), generator=g)
            if augment and mode == "random":
                torch.randint(0, n_ops, (len(LR),), generator=g)
        it_on = iter(on)
        for i, (l0, h0) in enumerate(off):
            l1, h1 = next(it_on)
            TN.assert_same_bits(h1, h0, "HR")
            if augment:
                assert torch.equal(on.last_index, off.last_index) and torch.equal(on.last_ops, off.last_ops)
            else:
                assert on.last_index is None and on.last_ops is None
            ids = order[4 * i:4 * i + 4].numpy()                        # the virtual index: (sample, op) j under "expand"
            want = Fh.taxel_noise(l0, sp, 8, epoch, ids=ids)
            TN.assert_same_bits(l1, want, "LR")
            assert not np.array_equal(l1.numpy(), l0.numpy())
            TN.check(l1.numpy(), l0.numpy(), TN.FULL, 8, epoch, ids, bar=TN.F32_BAR)
        assert torch.equal(on._gen.get_state(), off._gen.get_state()) and on.epoch == off.epoch == epoch
    TN.assert_same_bits(on.LR, LR, "the set itself stays clean")
    if mode == "expand":                                                # the views of one sample get different noise
        ld = DeviceSRLoader(LR, HR, 44, device="cpu", augment="rot90", augment_mode="expand",
                            taxel_noise=dict(sigma_add=1.0), noise_seed=8)
        (l, _), = list(ld)
        clean = torch.cat([b[0] for b in DeviceSRLoader(LR, HR, 44, device="cpu", augment="rot90", augment_mode="expand")])
        d = (l - clean).view(11, 4, -1)
        assert ld.last_index.tolist() == [j // 4 for j in range(44)]
        assert all(not torch.equal(d[:, a], d[:, b]) for a in range(4) for b in range(a))
        TN.assert_same_bits(l, Fh.taxel_noise(clean, dict(sigma_add=1.0), 8, 1))           # ids 0..43: the index j


def test_loader_noise_argument_checks():
    LR, HR = _set()
    for kw in (dict(taxel_noise="gauss"), dict(taxel_noise=dict(sigma_add=-1.0)), dict(taxel_noise=dict(axis_cnt=2))):
        with pytest.raises(ERR):
            DeviceSRLoader(LR, HR, 4, device="cpu", **kw)
    with pytest.raises(ERR):
        DeviceSRLoader(LR[:, 0], HR, 4, device="cpu", taxel_noise={})
    ld = DeviceSRLoader(LR, HR, 4, seed=12, device="cpu", taxel_noise={})
    assert ld.noise_seed == 12 and ld._noise.is_identity
    TN.assert_same_bits(torch.cat([b[0] for b in ld]), LR)
    assert DeviceSRLoader(LR, HR, 4, device="cpu", taxel_noise={}).noise_seed == 0


def test_tpsf_loader_reads_the_noise_keys():
    LR, HR = _set()
    assert D.tpsf_loader(LR, HR, {}, 4, device="cpu")._noise is None
    assert D.tpsf_loader(LR, HR, dict(taxel_noise=None, taxel_noise_seed=4), 4, device="cpu")._noise is None
    ld = D.tpsf_loader(LR, HR, dict(taxel_noise=dict(sigma_add=0.02), taxel_noise_seed=4), 4, device="cpu", seed=9)
    assert ld._noise == Fh.TaxelNoise(sigma_add=0.02) and ld.noise_seed == 4 and ld._ops is None
    TN.assert_same_bits(next(iter(ld))[0], Fh.taxel_noise(LR[:4], dict(sigma_add=0.02), 4, 1))
    ld = D.tpsf_loader(LR, HR, dict(taxel_noise=Fh.TaxelNoise(gain_jitter=0.1), is_aug_data=True), 4, device="cpu", seed=9)
    assert ld.noise_seed == 9 and ld._ops == (0, 1, 2, 3) and ld._noise.gain_jitter == np.float32(0.1)
    over = D.tpsf_loader(LR, HR, dict(taxel_noise=dict(sigma_add=0.02)), 4, device="cpu", taxel_noise=None)
    assert over._noise is None


class _Stub(torch.nn.Module):
    """A model eval_func can score without a GPU: the mean of the first frame's taxels, spread over the target's size."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(2.0))

    def forward(self, x):
        return (self.w * x[:, :3].mean(dim=(1, 2, 3), keepdim=True)).expand(-1, 1, 40, 40).contiguous()


def test_eval_func_keywords_and_default():
    sig = inspect.signature(TR.eval_func).parameters
    assert sig["taxel_noise"].default is None and sig["noise_seed"].default == 0
    assert list(sig)[:6] == ["model", "test_loader", "config", "windowed_ssim", "self_ensemble", "ema"]
    # the loop with taxel_noise=None is the parent's: scored on a stub with the device metrics replaced by torch ones
    conf = TR.default_config()
    g = torch.Generator().manual_seed(71)
    LR, HR = torch.rand(12, 3, 4, 4, generator=g) * 8, torch.rand(12, 1, 100, 100, generator=g) * 100
    seen = []

    class Spy(_Stub):
        def forward(self, x):
            seen.append(x.clone())
            return super().forward(x)
    saved = Fh.mse_loss, Fh.psnr_ssim, Fh.prepare_target
    Fh.mse_loss = lambda y, t: ((y - t) ** 2).mean()
    Fh.psnr_ssim = lambda y, t, m, reference_quirk=True: (-(y - t).abs().mean((1, 2, 3)), (y * t).mean((1, 2, 3)))
    Fh.prepare_target = lambda h, s, f: h[:, :, 30:70, 30:70] / s
    try:
        def run(bs, **kw):
            seen.clear()
            res = TR.eval_func(Spy(), DeviceSRLoader(LR, HR, bs, device="cpu"), conf, **kw)
            return res, torch.cat(seen)
        base, x0 = run(4)
        none, x1 = run(4, taxel_noise=None, noise_seed=5)
        assert none == base and len(base) == 3
        TN.assert_same_bits(x0, LR), TN.assert_same_bits(x1, LR)
        sp = _fh_spec(TN.FULL)
        a, xa = run(4, taxel_noise=sp, noise_seed=5)
        b, xb = run(3, taxel_noise=TN_dict(sp), noise_seed=5)
        TN.assert_same_bits(xa, Fh.taxel_noise(LR, sp, 5, 0)), TN.assert_same_bits(xb, xa)    # offset 0, ids = the running count
        assert a != base and all(abs(p - q) <= 1e-5 * abs(p) for p, q in zip(a, b))
        assert run(4, taxel_noise=sp, noise_seed=5)[0] == a                                 # deterministic
        assert run(4, taxel_noise=sp, noise_seed=6)[0] != a
    finally:
        Fh.mse_loss, Fh.psnr_ssim, Fh.prepare_target = saved


def TN_dict(t):
    return dict(sigma_add=t.sigma_add, sigma_mul=t.sigma_mul, gain_jitter=t.gain_jitter, drop_prob=t.drop_prob,
                drop_value=t.drop_value, axis_cnt=t.axis_cnt)
