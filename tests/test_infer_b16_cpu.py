"""CPU checks of tests/_infer_b16.py and of the host-side argument checks of the bf16-storage inference launches.

  * Refusals: every mutation of every table in _infer_b16 (`mutations`, `pack_mutations`) comes back as status exactly 1 from
    tsr_conv2d_fwd_b16, _b16k, _b16k_pair, _b16k_fuse1x1, tsr_conv2d_fwd, tsr_conv2d_fwd_bf16s, tsr_conv2d_ex and the pack
    routines.  The pointers are fake (never dereferenced); an argument list that is NOT refused reaches a launch, which without
    a device comes back as status 2.  tests/test_gpu_infer_b16.py sends the same tables to real buffers.
  * The host arithmetic of tsr_conv_weight_b16k_elems / _pair_elems.
  * The fp64 references equal torch compositions, `check_elements` finds a planted fault and names where it is, and every
    case table is well formed.
"""
import pytest
import torch
import torch.nn.functional as F

import _infer_b16 as S
from _infer_b16 import PAD, FAKE

KINDS = ["b16", "b16k", "pair", "fuse1x1"]


def fake_list(kind):
    v = S.valid_ints(kind)
    v.update({p: FAKE for p in S.POINTERS[kind]})
    return v


# ------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", KINDS + ["f32", "bf16s"])
def test_every_mutation_is_refused(kind):
    base = fake_list(kind)
    muts = S.mutations(kind)
    assert len({n for n, _ in muts}) == len(muts)
    for name, m in muts:
        assert all(k in base for k in m), (name, m)
        assert S.raw(kind, dict(base, **m)) == 1, f"{S.SIGS[kind][0]} accepted: {name}"
    if not torch.cuda.is_available():           # without a device the valid list passes every check and fails at the launch
        assert S.raw(kind, base) == 2


def test_every_mutation_of_conv2d_ex_is_refused():
    base = fake_list("ex")
    for name, m in S.mutations("ex"):
        assert S.raw_ex(dict(base, **m)) == 1, f"tsr_conv2d_ex accepted: {name}"
    if not torch.cuda.is_available():
        assert S.raw_ex(base) == 2
        assert S.raw_ex(dict(base, epi_mode=2, mask="res", mask_ctot=64 + PAD, mask_coff=16)) == 2      # (a valid mask slice)


def test_the_tables_hold_the_refusals_the_header_lists():
    for kind in KINDS:
        names = {n for n, _ in S.mutations(kind)}
        want = {"NULL in", "NULL w_packed", "NULL out", "B = 0", "H = -1", "W = 0", "cin = 0", "cin negative", "cin + 8", "in_coff 8",
                "in_ctot - 8", "out_ctot - 8", "out_coff 24", "in_coff negative", "out_coff negative", "in slice past the end",
                "out slice past the end"}
        if kind != "pair":
            want |= {"res_coff negative", "res slice past the end", "res_ctot - 8", "res_coff 8", "ks = 2", "ks = 7"}
        if kind != "b16":
            want |= {"cin odd multiple of 16", "32-bit halo offsets"}
        if kind in ("b16k", "fuse1x1"):
            want |= {"ks = 1"}
        if kind == "fuse1x1":
            want |= {"NULL w2_packed"}
        if kind in ("b16", "b16k"):
            want |= {"cout = 0", "cout = 32", "cout = 96", "cout = 256"}
        assert want <= names, (kind, want - names)
    assert "ks = 1" not in {n for n, _ in S.mutations("b16")}
    for kind in ("f32", "bf16s", "ex"):
        assert {"in_coff negative", "out_coff negative", "res_coff negative"} <= {n for n, _ in S.mutations(kind)}
    assert "mask_coff negative" in {n for n, _ in S.mutations("ex")}


@pytest.mark.parametrize("kind", ["pack_f32", "pack_bf16s", "pack_b16k", "pack_pair", "pack_w2"])
def test_pack_routines_refuse(kind):
    ints, muts = S.pack_mutations(kind)
    base = dict(ints, w=FAKE, w_packed=FAKE)
    for name, m in muts:
        assert S.raw(kind, dict(base, **m)) == 1, f"{S.SIGS[kind][0]} accepted: {name}"
    if not torch.cuda.is_available():
        assert S.raw(kind, base) == 2
    if kind in ("pack_f32", "pack_bf16s"):
        assert "cin = 0" in dict(muts) and "cin negative" in dict(muts)


def test_packed_weight_sizes():
    from tactilesr_amd._lib import load
    lib = load()
    for cout, cin, ks in [(64, 32, 3), (128, 96, 5), (64, 64, 1), (128, 448, 3), (64, 4096, 5)]:
        assert lib.tsr_conv_weight_b16k_elems(cout, cin, ks) == cout * cin * ks * ks
    for cin in (32, 64, 96, 128, 448, 4096):
        assert lib.tsr_conv_weight_b16k_pair_elems(cin) == (cin // 32) * 17 * 4096
        assert (cin // 32) * 17 * 4096 == 128 * cin * 9 + 64 * cin * 16        # 9 full inner taps + 16 outer taps of the 5x5 half


def test_abi_unchanged():
    from tactilesr_amd import _lib
    assert _lib.ABI_VERSION == 24 and _lib.load().tsr_abi_version() == 24
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "tactilesr_hip.h")) as f:
        header = f.read()
    assert "Refusals (status 1, nothing is launched, `out` is untouched) of tsr_conv2d_fwd_b16" in header
    assert "refuse (status 1, nothing launched) a NEGATIVE channel offset" in header


# ------------------------------------------------------------------------------------------------------- references
def _bn(y, s, t):
    return y * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)


def _q(t):
    return t.bfloat16().double()


def _r(t):
    return t.float().bfloat16().float()


def test_ref_b16_is_the_torch_composition():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 32, 9, 11, generator=g) * 3, torch.randn(64, 32, 5, 5, generator=g) * 0.1
    s, t, r = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g), torch.randn(2, 64, 9, 11, generator=g)
    conv = F.conv2d(_q(x), _q(w), padding=2)
    assert torch.equal(S.ref_b16(x, w), _r(conv))
    assert torch.equal(S.ref_b16(x, w, s, t, r, 1), _r(F.relu(_bn(conv, s, t) + _q(r))))
    assert torch.equal(S.ref_b16(x, w, None, t, None, 0), _r(conv + t.double().view(1, -1, 1, 1)))
    assert torch.equal(S.ref_b16(x, w, s, None, r, 0), _r(conv * s.double().view(1, -1, 1, 1) + _q(r)))
    got = S.ref_b16(x, w, s, t, r, 1)
    assert got.dtype == torch.float32 and torch.equal(got, got.bfloat16().float())       # bf16 values
    assert not torch.equal(S.ref_b16(x, w), _r(F.conv2d(x.double(), w.double(), padding=2)))  # (the operand rounding matters)


def test_ref_pair_b16_is_torch_cat_order():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 32, 7, 9, generator=g) * 3
    w3, w5 = torch.randn(64, 32, 3, 3, generator=g) * 0.1, torch.randn(64, 32, 5, 5, generator=g) * 0.1
    s, t = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    cat = torch.cat([F.conv2d(_q(x), _q(w3), padding=1), F.conv2d(_q(x), _q(w5), padding=2)], 1)
    assert torch.equal(S.ref_pair_b16(x, w3, w5), _r(cat))
    assert torch.equal(S.ref_pair_b16(x, w3, w5, s, t, 1), _r(F.relu(_bn(cat, s, t))))
    # the pair IS the 5x5 conv with cat([zero-padded 3x3 weight, 5x5 weight]) -- the weight the pack routine takes
    wc = S.pair_weight(w3, w5)
    assert wc.shape == (128, 32, 5, 5) and float(wc[:64, :, 0].abs().max()) == 0 and torch.equal(wc[:64, :, 1:4, 1:4], w3)
    assert torch.allclose(F.conv2d(_q(x), _q(wc), padding=2), cat, rtol=1e-13, atol=1e-13)
    assert torch.equal(S.ref_pair_b16(x, w3, w5, s, None, 0)[:, :64], S.ref_b16(x, w3, s[:64], None, None, 0))


def test_ref_fuse_b16_is_the_torch_composition():
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(2, 32, 6, 5, generator=g) * 3, torch.randn(128, 32, 3, 3, generator=g) * 0.1
    s, t = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.3
    w2, b2, r = torch.randn(64, 128, generator=g) * 0.1, torch.randn(64, generator=g), torch.randn(2, 64, 6, 5, generator=g)
    a = _r(F.relu(_bn(F.conv2d(_q(x), _q(w), padding=1), s, t))).double()               # the intermediate, rounded once
    want = F.relu(torch.einsum("oc,bchw->bohw", _q(w2), a) + b2.double().view(1, -1, 1, 1) + _q(r))
    assert torch.allclose(S.ref_fuse_b16(x, w, s, t, 1, w2, b2, r, 1).double(), _r(want).double(), rtol=2.0 ** -7, atol=1e-6)
    assert float((S.ref_fuse_b16(x, w, s, t, 1, w2, b2, r, 1) == _r(want)).float().mean()) > 0.999
    a0 = _r(F.conv2d(_q(x), _q(w), padding=1)).double()
    assert float((S.ref_fuse_b16(x, w, None, None, 0, w2) == _r(torch.einsum("oc,bchw->bohw", _q(w2), a0))).float().mean()) > 0.999


# ------------------------------------------------------------------------------------------------------- the checker
def _planted():
    g = torch.Generator().manual_seed(4)
    ref = (torch.randn(5, 64, 13, 21, generator=g) * 3).bfloat16().float()
    return ref, ref.clone()


def _ulp_up(v, n=1):
    """The bf16 value n steps away from zero from v."""
    return (v.bfloat16().view(torch.int16) + n).view(torch.bfloat16).float()


def test_check_elements_passes_the_untouched_tensor_and_counts_one_ulp_flips():
    ref, got = _planted()
    assert S.check_elements(got, ref, 1, 3e-6, 0.99) == (1.0, 0)
    got[0, 0, 0, :5] = _ulp_up(got[0, 0, 0, :5])
    same, off = S.check_elements(got, ref, 1, 3e-6, 0.99)
    assert off == 5 and same == 1.0 - 5 / ref.numel()
    assert 1.0 <= S.image_ratio(ref) < 4


def test_check_elements_finds_one_element():
    ref, got = _planted()
    got[3, 37, 9, 18] = _ulp_up(got[3, 37, 9, 18], 2)                # two ulps: beyond the one-ulp bar, within the two-ulp bar
    with pytest.raises(S.ElementMismatch) as ei:
        S.check_elements(got, ref, 1, 3e-6, 0.99)
    assert (ei.value.image, ei.value.tile, ei.value.block) == (3, (1, 2), 2)
    assert "image 3" in str(ei.value) and "block 2" in str(ei.value)
    S.check_elements(got, ref, 2, 2e-3, 0.98)


def test_check_elements_finds_one_image_slot():
    ref, got = _planted()
    got[4] = _ulp_up(got[4])                                        # all within one ulp, but a whole image differs: the share
    with pytest.raises(S.ElementMismatch) as ei:
        S.check_elements(got, ref, 1, 3e-6, 0.99)
    assert ei.value.image == 4 and "identical share" in str(ei.value)


def test_check_elements_finds_one_tile():
    ref, got = _planted()
    got[1, :, 8:13, 16:21] = _ulp_up(got[1, :, 8:13, 16:21], 3)      # the ragged corner tile
    with pytest.raises(S.ElementMismatch) as ei:
        S.check_elements(got, ref, 1, 3e-6, 0.99)
    assert (ei.value.image, ei.value.tile) == (1, (1, 2))


def test_check_elements_finds_one_channel_block():
    ref, got = _planted()
    got[2, 48:64] = _ulp_up(got[2, 48:64])                          # 1/20 of the tensor one ulp off
    with pytest.raises(S.ElementMismatch) as ei:
        S.check_elements(got, ref, 1, 3e-6, 0.99)
    assert (ei.value.image, ei.value.block) == (2, 3)
    ref, got = _planted()
    got[2, 48:64] *= 2                                              # (what a swapped default or a doubled half gives)
    with pytest.raises(S.ElementMismatch) as ei:
        S.check_elements(got, ref, 2, 2e-3, 0.98)
    assert (ei.value.image, ei.value.block) == (2, 3)


def test_check_elements_is_per_image_and_rejects_non_finite():
    ref, got = _planted()
    ref[0] *= 128                                                   # a tensor-wide floor would hide image 2 behind image 0
    got = ref.clone()
    small = ref[2].abs() < 0.01
    assert bool(small.any())
    b = int(small.flatten().nonzero()[0])
    delta = 1e-4 * float(ref[2].abs().max())
    got[2].view(-1)[b] += delta                                     # 3e-6 of the image's maximum < delta < 3e-6 of the tensor's
    assert 3e-6 * float(ref[2].abs().max()) < delta < 3e-6 * float(ref.abs().max())
    assert delta > 1.01 * 2.0 ** -7 * float(ref[2].view(-1)[b].abs())
    with pytest.raises(S.ElementMismatch) as ei:
        S.check_elements(got, ref, 1, 3e-6, 0.99)
    assert ei.value.image == 2
    ref, got = _planted()
    got[1, 20, 12, 0] = float("nan")
    with pytest.raises(S.ElementMismatch) as ei:
        S.check_elements(got, ref, 1, 3e-6, 0.99)
    assert (ei.value.image, ei.value.tile, ei.value.block) == (1, (1, 0), 1) and "non-finite" in str(ei.value)
    got[1, 20, 12, 0] = float("inf")
    with pytest.raises(S.ElementMismatch):
        S.check_elements(got, ref, 2, 2e-3, 0.98)


# ------------------------------------------------------------------------------------------------------- case tables
@pytest.mark.parametrize("name", list(S.TABLES))
def test_case_table_is_well_formed(name):
    cases = S.TABLES[name]
    for c in cases:
        offs = [o for _, _, o in S.case_slices(name, c)]
        assert len(set(offs)) == len(offs) and len(set(c.offs)) == len(c.offs), "every slice at a different offset"
        for width, ctot, coff in S.case_slices(name, c):
            assert width % 16 == 0 and ctot % 16 == 0 and coff % 16 == 0 and ctot == width + PAD
            assert 0 < coff and coff + width <= ctot
        assert c.H <= 40 and c.W <= 40 and c.B <= 74 and c.B * c.H * c.W <= 74 * 12 * 12, "nothing larger than 40x40 or B = 74 at 12x12"
        if name != "b16":
            assert c.cin % 32 == 0
    assert any(c.H < 8 and c.W < 8 for c in cases)
    assert any(c.H == 1 and c.W == 1 for c in cases)
    assert any(c.B == 1 and c.H < 8 and c.W < 8 for c in cases), "B = 1 in a 4-image workgroup with an image below one tile"
    assert {c.relu for c in cases} == {0, 1}
    assert {(c.scale, c.shift) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}
    assert {c.offs[0] for c in cases} == {16, 32, 48}
    if name in ("b16", "b16k"):
        assert {(c.res, c.relu) for c in cases} == {(True, 1), (True, 0), (False, 1), (False, 0)}
        assert any(S.case_grid(name, c) % 8 != 0 and S.case_grid(name, c) > 64 for c in cases), "a large grid that is no multiple of 8"
    else:
        assert any(S.case_grid(name, c) % 8 != 0 and S.case_grid(name, c) > 8 for c in cases)


def test_grids_follow_the_launchers():
    by = {(c.ks, c.cin, c.cout, c.B): S.case_grid("b16", c) for c in S.B16_CASES}
    assert by[(3, 64, 64, 5)] == 50 and by[(1, 256, 64, 3)] == 12 and by[(1, 64, 128, 70)] == 140 and by[(3, 128, 64, 74)] == 76
    assert by[(5, 128, 128, 6)] == 12 and by[(3, 448, 64, 1)] == 1
    by = {(c.ks, c.cin, c.cout, c.B): S.case_grid("b16k", c) for c in S.B16K_CASES}
    assert by[(3, 128, 128, 5)] == 50 and by[(3, 64, 64, 74)] == 76 and by[(5, 128, 64, 9)] == 18 and by[(5, 128, 128, 2)] == 6
    assert S.grid("pair", 37, 9, 17) == 60 and S.grid("fuse1x1", 5, 40, 40) == 50 and S.grid("b16", 3, 13, 21, ks=1) == 12
    assert 140 % 8 == 4 and 76 % 8 == 4 and 60 % 8 == 4


def test_the_ring_cases_reach_every_slot_phase():
    """Physical first row of block c = (c * HH) & 15: 8 phases for 3x3 (HH = 10), 4 for 5x5 (HH = 12)."""
    assert S.ring_rows(3, 256) == [0, 10, 4, 14, 8, 2, 12, 6] and S.ring_rows(3, 512)[8:] == S.ring_rows(3, 256)
    assert S.ring_rows(5, 128) == [0, 12, 8, 4] and S.ring_rows(5, 256)[4:] == S.ring_rows(5, 128)
    assert any(c.ks == 3 and c.cin >= 256 for c in S.B16K_CASES) and any(c.ks == 5 and c.cin >= 128 for c in S.B16K_CASES)


def test_the_issue_s_shapes_are_all_there():
    f = {(c.ks, c.cin, c.cout, c.B, c.H, c.W) for c in S.B16_CASES}
    assert f >= {(3, 64, 64, 5, 40, 40), (1, 256, 64, 3, 13, 21), (5, 48, 128, 2, 5, 3), (3, 16, 64, 1, 1, 1), (3, 192, 64, 1, 8, 8),
                 (1, 64, 128, 70, 12, 12), (3, 128, 64, 74, 12, 12), (5, 128, 128, 6, 13, 21), (3, 448, 64, 1, 8, 8)}
    f = {(c.ks, c.cin, c.cout, c.B, c.H, c.W) for c in S.B16K_CASES}
    assert f >= {(3, 128, 128, 5, 40, 40), (5, 128, 128, 2, 13, 21), (3, 32, 64, 1, 1, 1), (5, 96, 128, 3, 5, 3), (5, 64, 128, 1, 3, 5),
                 (3, 64, 64, 74, 12, 12), (3, 256, 128, 1, 8, 8), (5, 128, 64, 9, 9, 17)}
    p = S.PAIR_CASES
    assert {c.cin for c in p} == {32, 64, 96, 128} and {c.B for c in p} == {1, 3, 5, 37}
    assert {(c.H, c.W) for c in p} == {(1, 1), (5, 3), (9, 17), (13, 21), (40, 40)}
    assert {(c.cin, c.B, c.H, c.W) for c in p} >= {(64, 3, 40, 40), (32, 37, 9, 17)}
    u = S.FUSE_CASES
    assert {c.ks for c in u} == {3, 5} and {c.cin for c in u} == {32, 96, 128} and {c.B for c in u} == {1, 2, 5}
    assert {(c.H, c.W) for c in u} == {(1, 1), (5, 3), (13, 21), (40, 40)} and {c.relu for c in u} == {0, 1}
    assert len({(c.shift2, c.res, c.relu2) for c in u}) == 8
    assert {(c.ks, c.cin, c.shift2, c.res, c.relu2) for c in u} >= {(3, 128, True, True, 0), (5, 128, False, True, 1)}


@pytest.mark.parametrize("name", list(S.TABLES))
def test_images_of_a_case_have_one_magnitude(name):
    """max_b max|ref_b| / min_b max|ref_b| < 4 for every case: the per-image floor is the tensor-wide floor up to that factor.
    (The GPU tests assert it again on the reference they compare with.)"""
    inputs, ref = S.INPUTS[name]
    for c in S.TABLES[name]:
        r = ref(inputs(c))
        assert torch.isfinite(r).all() and S.image_ratio(r) < 4, (c, S.image_ratio(r))
