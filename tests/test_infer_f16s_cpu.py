"""CPU checks of tests/_infer_f16s.py: the fp64 references of tests/test_gpu_infer_fp16x3.py agree with torch compositions, the
per-image checker finds a planted fault and names where it is, and every case table is well formed (slices inside their
buffers, an image below one tile, a grid that is no multiple of 8, images of one magnitude).

Refusals: every mutation in _infer_f16s of the three fp16x3 launches, of their pack routines and of the five dgrad pack
routines comes back as status exactly 1.  The pointers are fake (never dereferenced); an argument list that is NOT refused
reaches a launch, which without a device comes back as status 2.  tests/test_gpu_infer_fp16x3.py sends the launch and pack
tables to real buffers."""
import pytest
import torch
import torch.nn.functional as F

import _infer_f16s as S


def _bn(y, s, t):
    return y * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)


def test_ref_conv_is_the_torch_composition():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 32, 9, 11, generator=g), torch.randn(64, 32, 5, 5, generator=g) * 0.1
    s, t, r = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g), torch.randn(2, 64, 9, 11, generator=g)
    conv = F.conv2d(x.double(), w.double(), padding=2)
    assert torch.equal(S.ref_conv(x, w), conv)
    assert torch.allclose(S.ref_conv(x, w, s, t, r, 1), F.relu(_bn(conv, s, t) + r.double()), rtol=1e-14, atol=0)
    assert torch.allclose(S.ref_conv(x, w, None, t, None, 0), conv + t.double().view(1, -1, 1, 1), rtol=1e-14, atol=0)
    assert torch.allclose(S.ref_conv(x, w, s, None, r, 0), conv * s.double().view(1, -1, 1, 1) + r.double(), rtol=1e-14, atol=0)
    assert S.ref_conv(x, w).dtype == torch.float64


def test_pair_perm_and_ref_pair():
    perm = S.pair_perm()
    assert sorted(perm.tolist()) == list(range(128))
    # every wave half (64 kernel channels) holds two 16-channel blocks of each conv
    for wn in range(2):
        half = perm[wn * 64:(wn + 1) * 64]
        assert sorted(half[:32].tolist()) == list(range(wn * 32, wn * 32 + 32))
        assert sorted(half[32:].tolist()) == list(range(64 + wn * 32, 64 + wn * 32 + 32))
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 16, 7, 9, generator=g)
    w3, w5 = torch.randn(64, 16, 3, 3, generator=g) * 0.1, torch.randn(64, 16, 5, 5, generator=g) * 0.1
    s, t = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    cat = torch.cat([F.conv2d(x.double(), w3.double(), padding=1), F.conv2d(x.double(), w5.double(), padding=2)], 1)
    got = S.ref_pair(x, w3, w5, s, t, 1)
    for k in range(128):        # kernel channel k = logical channel perm[k], with the k-th scale / shift
        want = F.relu(cat[:, perm[k]] * float(s[k].double()) + float(t[k].double()))
        assert torch.allclose(got[:, k], want, rtol=1e-14, atol=0)
    assert torch.equal(S.ref_pair(x, w3, w5), cat[:, perm])


def test_ref_fuse1x1_is_the_torch_composition():
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(2, 16, 6, 5, generator=g), torch.randn(128, 16, 3, 3, generator=g) * 0.1
    s, t = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.3
    w2, b2, r = torch.randn(64, 128, 1, 1, generator=g) * 0.1, torch.randn(64, generator=g), torch.randn(2, 64, 6, 5, generator=g)
    a = F.relu(_bn(F.conv2d(x.double(), w.double(), padding=1), s, t))
    want = F.relu(F.conv2d(a, w2.double(), b2.double()) + r.double())
    assert torch.allclose(S.ref_fuse1x1(x, w, s, t, 1, w2, b2, r, 1), want, rtol=1e-13, atol=1e-13)
    a0 = F.conv2d(x.double(), w.double(), padding=1)
    assert torch.allclose(S.ref_fuse1x1(x, w, None, None, 0, w2), F.conv2d(a0, w2.double()), rtol=1e-13, atol=1e-13)
    # the model's two-launch chain is the 1x1 `confusion` over cat([stage 3x3, stage 5x5]) + bias + x, ReLU
    w5 = torch.randn(128, 16, 5, 5, generator=g) * 0.05
    wb = torch.randn(64, 128, 1, 1, generator=g) * 0.1
    P = S.ref_fuse1x1(x, w, s, t, 1, w2, b2, r, 0)
    out = S.ref_fuse1x1(x, w5, s, t, 1, wb, None, P, 1)
    a5 = F.relu(_bn(F.conv2d(x.double(), w5.double(), padding=2), s, t))
    whole = F.relu(F.conv2d(torch.cat([a, a5], 1), torch.cat([w2, wb], 1).double(), b2.double()) + r.double())
    assert torch.allclose(out, whole, rtol=1e-12, atol=1e-12)


def test_host_wscale():
    for mx, want in [(0.25, 2.0 ** 15), (0.2345, 2.0 ** 16), (1.0 - 2.0 ** -24, 2.0 ** 14), (1.0, 2.0 ** 13), (3.0, 2.0 ** 12)]:
        w = torch.tensor([0.01, -mx])
        ws = S.host_wscale(w)
        assert ws == want and 2.0 ** 13 <= mx * ws < 2.0 ** 14
    assert S.host_wscale(torch.tensor([0.1]), torch.tensor([-0.9])) == 2.0 ** 14
    assert S.host_wscale(torch.zeros(3)) == 1.0


# ------------------------------------------------------------------------------------------------------- the checker
def _planted():
    g = torch.Generator().manual_seed(4)
    ref = torch.randn(5, 64, 13, 21, generator=g, dtype=torch.float64) * 3
    return ref, ref.float()


def test_check_images_passes_the_untouched_tensor():
    ref, got = _planted()
    per = S.check_images(got, ref)
    assert per.shape == (5,) and float(per.max()) < 1e-6
    assert 1.0 <= S.image_ratio(ref) < 4


def test_check_images_finds_one_element():
    ref, got = _planted()
    got[3, 37, 9, 18] += 3e-5 * float(ref[3].abs().max())
    with pytest.raises(S.ImageMismatch) as ei:
        S.check_images(got, ref)
    assert (ei.value.image, ei.value.tile, ei.value.block) == (3, (1, 2), 2)
    assert "image 3" in str(ei.value) and "block 2" in str(ei.value)


def test_check_images_finds_one_image_slot():
    ref, got = _planted()
    got[4] += 3e-5 * float(ref[4].abs().max())
    with pytest.raises(S.ImageMismatch) as ei:
        S.check_images(got, ref)
    assert ei.value.image == 4


def test_check_images_finds_one_tile():
    ref, got = _planted()
    got[1, :, 8:13, 16:21] += 3e-5 * float(ref[1].abs().max())       # the ragged corner tile
    with pytest.raises(S.ImageMismatch) as ei:
        S.check_images(got, ref)
    assert (ei.value.image, ei.value.tile) == (1, (1, 2))


def test_check_images_finds_one_channel_block():
    ref, got = _planted()
    got[2, 48:64] += 3e-5 * float(ref[2].abs().max())
    with pytest.raises(S.ImageMismatch) as ei:
        S.check_images(got, ref)
    assert (ei.value.image, ei.value.block) == (2, 3)


def test_check_images_is_per_image_and_rejects_non_finite():
    ref, got = _planted()
    ref[0] *= 100                                            # a tensor-wide max-norm would hide image 2 behind image 0
    got = ref.float()
    got[2, 5, 1, 1] += 3e-5 * float(ref[2].abs().max())
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < S.TOL
    with pytest.raises(S.ImageMismatch) as ei:
        S.check_images(got, ref)
    assert ei.value.image == 2
    ref, got = _planted()
    got[1, 20, 12, 0] = float("nan")
    with pytest.raises(S.ImageMismatch) as ei:
        S.check_images(got, ref)
    assert (ei.value.image, ei.value.tile, ei.value.block) == (1, (1, 0), 1)


# ------------------------------------------------------------------------------------------------------- case tables
TABLES = {"f16s": S.F16S_CASES, "pair": S.PAIR_CASES, "fuse1x1": S.FUSE_CASES}


@pytest.mark.parametrize("name", list(TABLES))
def test_case_table_is_well_formed(name):
    cases = TABLES[name]
    for c in cases:
        offs = [o for _, _, o in S.case_slices(c)]
        assert len(set(offs)) == len(offs) and len(set(c.offs)) == len(c.offs), "every slice at a different offset"
        for width, ctot, coff in S.case_slices(c):
            assert width % 16 == 0 and ctot % 16 == 0 and coff % 16 == 0 and ctot == width + S.PAD
            assert 0 < coff and coff + width <= ctot
        assert c.amax in (None, "zero", "big", "half")
    assert any(c.H < 8 and c.W < 8 for c in cases)
    assert any(c.H == 1 and c.W == 1 for c in cases)
    assert any(S.case_grid(c) % 8 != 0 and S.case_grid(c) > 64 for c in cases), "a large grid that is no multiple of 8"
    assert {c.amax for c in cases} == {None, "zero", "big", "half"}
    assert {c.relu for c in cases} == {0, 1}
    assert {(c.scale, c.shift) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}


def test_grids_follow_the_launchers():
    by = {(c.ks, c.cin, c.cout, c.B): S.case_grid(c) for c in S.F16S_CASES}
    assert by[(3, 128, 64, 70)] == 72 and by[(3, 128, 64, 74)] == 76 and by[(1, 64, 64, 70)] == 140
    assert by[(3, 64, 64, 3)] == 25 and by[(5, 64, 128, 3)] == 50 and by[(1, 256, 64, 5)] == 18
    assert S.grid("pair", 37, 9, 17) == 114 and S.grid("fuse1x1", 5, 40, 40) == 75
    assert {c.ks for c in S.F16S_CASES} == {1, 3, 5} and {c.cout for c in S.F16S_CASES} == {64, 128}


def test_the_issue_s_shapes_are_all_there():
    f = {(c.ks, c.cin, c.cout, c.B, c.H, c.W) for c in S.F16S_CASES}
    assert f >= {(3, 64, 64, 3, 40, 40), (5, 128, 128, 2, 13, 21), (1, 256, 64, 5, 9, 17), (3, 16, 128, 1, 5, 3),
                 (5, 48, 64, 2, 1, 1), (1, 128, 128, 3, 13, 21), (3, 128, 64, 70, 12, 12), (1, 64, 64, 70, 12, 12),
                 (5, 64, 128, 3, 40, 40), (3, 448, 64, 1, 8, 8), (1, 64, 128, 1, 1, 1)}
    assert {(c.res, c.relu) for c in S.F16S_CASES} == {(True, 1), (True, 0), (False, 1), (False, 0)}
    p = S.PAIR_CASES
    assert {c.cin for c in p} == {16, 32, 48, 64, 128} and {c.B for c in p} >= {1, 3, 5}
    assert {(c.H, c.W) for c in p} == {(1, 1), (5, 3), (9, 17), (13, 21), (40, 40)}
    u = S.FUSE_CASES
    assert {c.ks for c in u} == {3, 5} and {c.cin for c in u} == {16, 48, 128} and {c.B for c in u} == {1, 2, 5}
    assert {(c.H, c.W) for c in u} == {(1, 1), (5, 3), (13, 21), (40, 40)}
    assert len({(c.shift2, c.res, c.relu2) for c in u}) == 8


@pytest.mark.parametrize("name", list(TABLES))
def test_images_of_a_case_have_one_magnitude(name):
    """max_b max|ref_b| / min_b max|ref_b| < 4 for every case: the per-image bar is the tensor-wide bar up to that factor.
    (The GPU tests assert it again on the reference they compare with.)"""
    inputs, ref = {"f16s": (S.f16s_inputs, S.f16s_ref), "pair": (S.pair_inputs, S.pair_ref), "fuse1x1": (S.fuse_inputs, S.fuse_ref)}[name]
    for c in TABLES[name]:
        r = ref(inputs(c))
        assert S.image_ratio(r) < 4, (c, S.image_ratio(r))
        prior = S.amax_prior(c.amax, r)
        if c.amax == "big":
            assert float(r.abs().max()) * 2 < prior
        if c.amax == "half":
            assert 0 < prior < float(r.abs().max())


# ------------------------------------------------------------------------------------------------------- refusals
def _refused(name, sig, base, muts):
    for m in muts:
        assert all(k in base for k in m), (name, m)
        assert S.raw_fake(name, sig, dict(base, **m)) == 1, f"{name} accepted: {m}"
    if not torch.cuda.is_available():           # without a device the valid list passes every check and fails at the launch
        assert S.raw_fake(name, sig, base) == 2


@pytest.mark.parametrize("kind", list(S.LAUNCHES))
def test_every_mutation_is_refused(kind):
    name, sig = S.LAUNCHES[kind]
    muts = S.launch_mutations(kind)
    assert len({repr(m) for m in muts}) == len(muts)
    _refused(name, sig, S.fake_launch_args(kind), muts)


def test_the_launch_tables_hold_every_refusal():
    for kind in S.LAUNCHES:
        muts = S.launch_mutations(kind)
        want = [{"in": None}, {"w_packed": None}, {"out": None}, {"in_amax": None}, {"B": 0}, {"H": -1}, {"W": 0}, {"cin": 0},
                {"cin": -16}, {"cin": 24}, {"in_coff": 8}, {"in_coff": -16}, {"out_coff": -16}, {"out_coff": 24}]
        want += [{"w_inv_scale": v} for v in (0.0, -1.0)]
        if kind != "pair":
            want += [{"res_coff": -16}, {"res_coff": 8}, {"ks": 2}, {"ks": 7}]
        if kind == "fuse1x1":
            want += [{"w2_packed": None}, {"ks": 1}, {"w2_inv_scale": 0.0}]
        if kind == "f16s":
            want += [{"cout": 0}, {"cout": 96}]
        assert all(w in muts for w in want), (kind, [w for w in want if w not in muts])
        assert sum(1 for m in muts if any(isinstance(v, float) and v != v for v in m.values())) == (2 if kind == "fuse1x1" else 1)
    assert {"ks": 1} not in S.launch_mutations("f16s")


@pytest.mark.parametrize("cout,cin,ks", S.PACK_SHAPES)
def test_pack_routines_refuse(cout, cin, ks):
    ints = dict(w=S.FAKE, w_packed=S.FAKE, cout=cout, cin=cin, ks=ks)
    _refused("tsr_pack_conv_weight_f16s", S.PACK_SIG, dict(ints, wscale=2.0 ** 14), S.pack_host_mutations(cin))
    _refused("tsr_pack_conv_weight_f16s_dev", S.PACK_DEV_SIG, dict(ints, w_amax=S.FAKE), S.pack_dev_mutations(cin))


def test_pair_pack_refuses():
    cin = S.PACK_PAIR_CIN
    base = dict(w3=S.FAKE, w5=S.FAKE, w_packed=S.FAKE, cin=cin, wscale=2.0 ** 14, w_amax=None)
    _refused("tsr_pack_conv_weight_pair_f16s", S.PACK_PAIR_SIG, base, S.pack_pair_mutations(cin))
    if not torch.cuda.is_available():
        assert S.raw_fake("tsr_pack_conv_weight_pair_f16s", S.PACK_PAIR_SIG, dict(base, wscale=0.0, w_amax=S.FAKE)) == 2   # w_amax replaces wscale


@pytest.mark.parametrize("name", list(S.DGRAD_PACK_SIGS))
def test_dgrad_pack_routines_refuse(name):
    """NULL pointers, cout not a multiple of 16, nprime not 64 / 128, ci0 < 0, ci0 + nprime > cin, a bad ks."""
    sig = S.DGRAD_PACK_SIGS[name]
    base = dict(S.DGRAD_PACK_VALID, w=S.FAKE, w_packed=S.FAKE, w_amax=S.FAKE)
    _refused(name, sig, base, S.dgrad_pack_mutations(name))
    if not torch.cuda.is_available():
        assert S.raw_fake(name, sig, dict(base, nprime=64, ci0=128)) == 2            # the other width, ending the buffer
    if "wscale:f" in sig:
        for v in S.BAD_SCALES:
            assert S.raw_fake(name, sig, dict(base, wscale=v)) == 1, v
    if "nsplit:i" in sig:
        for v in (0, 4, -1):
            assert S.raw_fake(name, sig, dict(base, nsplit=v)) == 1, v
