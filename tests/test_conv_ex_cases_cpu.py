"""CPU checks of tests/_conv_ex_cases.py: the tables of tests/test_gpu_conv_ex.py moved there unchanged, the rows added for the
conv_b16k / conv1x1_b16k launches are the ones their docstring names, the fp64 references agree with torch (autograd for the
data gradient), the slab checkers find a planted wrong entry, a wrong count in an absent image's slot and a write into the guard
band, and the conditions that keep the GPU comparisons honest hold for the seeded inputs of the new rows (tensor sizes for
the 99 % share, the share of mask pre-activations next to zero).

Refusals: every mutation of `_conv_ex_cases.MUTATIONS` comes back from `tsr_conv2d_ex` as status exactly 1.  The pointers are
fake (never dereferenced): a descriptor that is NOT refused reaches a launch, which without a device comes back as status 2.
tests/test_gpu_conv_ex_b16k.py sends the same table to real buffers."""
import pytest
import torch
import torch.nn.functional as F

import _conv_ex_cases as C


# ---------------------------------------------------------------------------------------------------------------- tables
def test_the_moved_tables_are_what_test_gpu_conv_ex_held():
    assert C.FWD1_CASES == [
        (3, 64, 64, 3, 40, 40, True, 16, 32, 0.0),
        (5, 128, 128, 2, 13, 21, True, 32, 16, 1.0e6),
        (1, 256, 64, 5, 9, 17, True, 16, 16, None),
        (3, 16, 128, 1, 5, 3, False, 32, 32, 0.0),
        (5, 48, 64, 2, 1, 1, True, 16, 32, None),
        (1, 128, 128, 3, 13, 21, False, 32, 16, 0.0),
        (3, 128, 64, 70, 12, 12, False, 16, 32, None),
        (5, 64, 128, 3, 40, 40, False, 16, 16, 0.0),
        (3, 256, 128, 2, 9, 17, True, 32, 16, None),
        (1, 64, 64, 1, 40, 40, True, 16, 32, 0.0),
    ]
    assert C.FWD0_CASES == [
        (1, 256, 64, 2, 40, 40, True, "plain", 1, False, 16, 32, 16),
        (1, 256, 64, 3, 13, 21, True, "virtual", 1, False, 32, 16, 32),
        (3, 64, 64, 5, 9, 17, False, "plain", 1, False, 16, 32, 0),
        (3, 64, 64, 1, 5, 3, False, None, 1, False, 32, 16, 0),
        (1, 128, 128, 2, 1, 1, True, None, 0, False, 16, 32, 0),
        (5, 48, 128, 3, 13, 21, True, "virtual", 0, True, 32, 16, 32),
        (5, 16, 64, 2, 9, 17, False, "plain", 0, False, 16, 16, 32),
        (1, 64, 64, 70, 12, 12, False, "plain", 1, False, 32, 32, 16),
        (3, 128, 128, 2, 40, 40, True, "plain", 1, False, 16, 32, 32),
    ]
    assert C.DGRAD_CASES == [
        (3, 64, 64, 64, 0, 3, 40, 40, True, "bn", False, 16, 32, 16, 32),
        (5, 128, 192, 128, 64, 2, 13, 21, True, "bn", True, 32, 16, 32, 16),
        (1, 64, 256, 128, 128, 5, 9, 17, False, "bn", False, 16, 16, 0, 32),
        (3, 16, 64, 64, 0, 1, 5, 3, True, "bn", False, 32, 32, 16, 16),
        (5, 48, 128, 64, 64, 2, 1, 1, True, "mask", False, 16, 32, 32, 16),
        (1, 256, 64, 64, 0, 3, 13, 21, False, "partial", True, 32, 16, 0, 0),
        (3, 128, 128, 128, 0, 70, 12, 12, True, "bn", False, 16, 32, 32, 16),
        (5, 64, 64, 64, 0, 3, 40, 40, True, "partial", False, 16, 16, 32, 0),
        (3, 256, 128, 128, 0, 2, 9, 17, True, "bn", False, 32, 16, 0, 48),
        (1, 128, 128, 64, 64, 1, 40, 40, True, "bn", False, 16, 32, 16, 32),
    ]
    import test_gpu_conv_ex as G
    assert G.FWD1_CASES is C.FWD1_CASES and G.FWD0_CASES is C.FWD0_CASES and G.DGRAD_CASES is C.DGRAD_CASES
    assert G.IMPLS == {"f32": 0, "bf16x6": 3, "fp16x3": -2, "bf16op": 1, "bf16x3": 2, "bf16": -1}
    assert G.TOL == {0: 1e-5, 3: 1e-5, -2: 1e-5, 1: 1e-5, 2: 1e-4, -1: 1e-5}
    assert G.SUM_TOL == {0: 1e-5, 3: 1e-5, -2: 1e-5, 1: 1e-5, 2: 1e-4, -1: 1e-4} and G.GUARD == 8
    assert (C.NS_B16K, C.NS_B16K_PAIR) == (-3, -4)


def _has(table, **want):
    names = {"fwd1": "ks cin cout B H W virt in_coff out_coff prior", "fwd0": "ks cin cout B H W virt res relu scale in_coff out_coff res_coff",
             "dgrad": "ks K cin_f N ci0 B H W res form scale in_coff out_coff res_coff mask_coff", "pair": "cin B H W virt in_coff out_coff"}
    f = names[table].split()
    return any(all(r[f.index(k)] == v for k, v in want.items()) for r in C.TABLES[table])


def test_every_shape_the_b16k_tests_name_is_present():
    assert _has("fwd1", ks=3, cin=32, cout=128, B=1, H=5, W=3, virt=False)
    assert _has("fwd1", ks=5, cin=32, cout=64, B=5, H=1, W=1)
    assert _has("fwd1", ks=5, cin=96, cout=128, B=6, H=13, W=21)
    assert _has("pair", cin=32, B=1, H=1, W=1) and _has("pair", cin=96, B=5, H=13, W=21) and _has("pair", cin=64, B=70, H=12, W=12)
    assert _has("fwd0", ks=3, cin=128, cout=128, B=3, H=9, W=17, res="plain", relu=0, scale=True, virt=False)
    assert _has("fwd0", ks=3, cin=64, cout=64, res="plain") and _has("fwd0", ks=3, cin=64, cout=64, res=None)
    assert _has("fwd0", ks=1, cin=128, cout=64, B=1, H=1, W=1, virt=True)
    assert _has("fwd0", ks=1, cin=256, cout=64, B=3, H=5, W=3, virt=True, res="virtual")
    assert _has("dgrad", ks=5, K=32, N=64, ci0=64, B=5, H=1, W=1, res=True, scale=True, form="bn")
    assert _has("dgrad", ks=3, K=96, N=128, B=6, H=13, W=21, res=True, form="bn")
    assert _has("dgrad", ks=1, K=64, N=128, B=3, H=5, W=3, form="bn")
    assert any(r[9] == "mask" and C.b16k_accepts("dgrad", r) and r[0] > 1 for r in C.TABLES["dgrad"])
    assert any(r[9] == "mask" and C.b16k_accepts("dgrad", r) and r[0] == 1 for r in C.TABLES["dgrad"])
    for kind, rows in C.TABLES.items():
        assert len(set(rows)) == len(rows)
        for r in rows:
            B, H, W = (r[1:4] if kind == "pair" else (r[5:8] if kind == "dgrad" else r[3:6]))
            assert B <= 70 and H <= 40 and W <= 40


def test_res_mask_and_out_of_the_k96_dgrad_row_differ_in_ctot_and_coff():
    row = next(r for r in C.B16K_DGRAD_CASES if r[1] == 96)
    P = C.make_problem("dgrad", row)
    d = C.desc_ints(P, C.NS_B16K)
    assert len({d["out_ctot"], d["res_ctot"], d["mask_ctot"], d["in_ctot"]}) == 4
    assert len({d["out_coff"], d["res_coff"], d["mask_coff"]}) == 3
    assert len(set(C.PADS.values())) == 4


def test_slices_stay_inside_their_buffers():
    for kind, rows in C.TABLES.items():
        for r in rows:
            offs = {"fwd1": r[7:9], "fwd0": r[10:13], "dgrad": r[11:15], "pair": r[5:7]}[kind]
            for name, o in zip(("in", "out", "res", "mask"), offs):
                assert o % 16 == 0 and 0 <= o <= C.PADS[name]


def test_b16k_accepts_row_by_row():
    acc = lambda kind, rows: [C.b16k_accepts(kind, r) for r in rows]
    assert acc("fwd1", C.FWD1_CASES) == [True, True, False, False, False, False, True, True, True, False]
    assert acc("fwd0", C.FWD0_CASES) == [True, True, True, True, False, False, False, False, True]
    assert acc("dgrad", C.DGRAD_CASES) == [True, True, True, False, False, False, True, True, True, False]
    for kind, rows in (("fwd1", C.B16K_FWD1_CASES), ("fwd0", C.B16K_FWD0_CASES), ("dgrad", C.B16K_DGRAD_CASES), ("pair", C.PAIR_CASES)):
        assert all(acc(kind, rows)), kind
    # one condition at a time, from an accepted row
    assert not C.b16k_accepts("fwd0", (3, 64, 64, 5, 9, 17, False, "virtual", 1, False, 16, 32, 0))
    assert not C.b16k_accepts("fwd0", (1, 256, 64, 2, 40, 40, False, "plain", 1, False, 16, 32, 16))
    assert not C.b16k_accepts("fwd0", (1, 256, 64, 2, 40, 40, True, "plain", 1, True, 16, 32, 16))
    assert not C.b16k_accepts("fwd0", (1, 64, 64, 2, 40, 40, True, "plain", 1, False, 16, 32, 16))
    assert not C.b16k_accepts("dgrad", (1, 64, 256, 128, 128, 5, 9, 17, True, "bn", False, 16, 16, 0, 32))
    assert not C.b16k_accepts("dgrad", (1, 64, 256, 128, 128, 5, 9, 17, False, "bn", True, 16, 16, 0, 32))
    assert not C.b16k_accepts("dgrad", (1, 64, 256, 128, 128, 5, 9, 17, False, "partial", False, 16, 16, 0, 32))


# ---------------------------------------------------------------------------------------------------------------- references
def test_dgrad_reference_is_autograd_of_the_forward_conv():
    row = (3, 32, 64, 64, 0, 2, 5, 3, True, "bn", True, 16, 32, 48, 16)
    P = C.make_problem("dgrad", row, 0)
    g = torch.Generator().manual_seed(3000 + 3 * 7 + 32 + 64 + 2 + 5)
    dz = torch.randn(2, 32, 5, 3, generator=g)
    w = torch.randn(32, 64, 3, 3, generator=g) * 0.05
    assert torch.equal(dz, P["z"]) and torch.equal(w, P["w"])
    x = torch.zeros(2, 64, 5, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, w.double(), padding=1) * dz.double()).sum().backward()
    want = x.grad * P["scale"].double().view(1, -1, 1, 1) + P["r"].double()
    assert torch.allclose(P["ref"], want, rtol=1e-12, atol=1e-12)
    exp, share = C.dgrad_expected(P, want.float())
    on = P["pre"] > 0
    assert share == 0.0 and torch.equal(exp, torch.where(on, P["ref"], torch.zeros_like(P["ref"])))
    assert 0.2 < float(on.double().mean()) < 0.8


def test_forward_references_are_the_torch_compositions():
    P = C.make_problem("fwd0", (3, 32, 64, 2, 5, 3, True, "virtual", 1, True, 16, 32, 48))
    a = C.q16(F.relu(C.fma32(P["z"], P["s"], P["t"]))).double()
    assert torch.equal(P["z"], C.q16(P["z"])) and torch.equal(C.materialised(P), a.float())
    y = F.conv2d(a, C.q16(P["w"]).double(), padding=1) * P["scale"].double().view(1, -1, 1, 1) + P["shift"].double().view(1, -1, 1, 1)
    y = F.relu(y + F.relu(C.fma32(P["r"], P["rs"], P["rt"])).double())
    assert torch.equal(P["ref"], y)
    Q = C.make_problem("pair", (32, 2, 5, 3, False, 16, 32))
    w3, w5 = Q["w"][:64, :, 1:4, 1:4], Q["w"][64:]
    assert torch.equal(Q["w"][:64], F.pad(w3, (1, 1, 1, 1)))                       # the 3x3 half is zero outside its taps
    want = torch.cat([F.conv2d(Q["z"].double(), C.q16(w3).double(), padding=1), F.conv2d(Q["z"].double(), C.q16(w5).double(), padding=2)], 1)
    assert torch.equal(Q["ref"], want)
    assert torch.allclose(Q["ref"], F.conv2d(Q["z"].double(), C.q16(Q["w"]).double(), padding=2), rtol=1e-12, atol=1e-12)


def test_streamed_entry_sums_are_those_of_the_persistent_loop_tests():
    import _persistent_loops as PL
    g = torch.Generator().manual_seed(4)
    x, h = torch.randn(3, 128, 5, 3, generator=g).double(), torch.randn(3, 128, 5, 3, generator=g).double()
    grid, per = C.dgrad1x1_split(3, 5, 3)
    assert (grid, per) == (3, 1) == PL.split(3 * 1, PL.DGRAD1X1_CAP)
    got = C.streamed_entry_sums(x, h, grid, per)
    assert torch.equal(got[:, :, 0], PL.entry_sums(x, grid, per)) and torch.equal(got[:, :, 1], PL.entry_sums(x * h, grid, per))
    assert C.dgrad1x1_split(5000, 5, 7) == PL.split(5000 * 3, PL.DGRAD1X1_CAP) == (2048, 8)


# ---------------------------------------------------------------------------------------------------------------- checkers
def _welford_slabs(ref, img):
    B, cout, H, W = ref.shape
    entries, cnt = C.entry_counts(img, B, H, W)
    slab = torch.full((entries + C.GUARD, cout, 2), C.NAN)
    for e in range(entries):
        b, y0, x0 = C.entry_image_tile(e, img, B, H, W)
        if b >= B:
            slab[e] = 0.0
            continue
        t = ref[b, :, y0:y0 + 8, x0:x0 + 8].reshape(cout, -1)
        slab[e, :, 0], slab[e, :, 1] = t.mean(1).float(), ((t - t.mean(1, keepdim=True)) ** 2).sum(1).float()
    return slab.reshape(-1), torch.cat([cnt.float(), torch.full((C.GUARD,), C.NAN)]), entries


def test_check_welford_finds_a_wrong_entry_a_wrong_absent_count_and_a_guard_write():
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(5, 64, 13, 21, generator=g).double()
    slab, cnt, entries = _welford_slabs(ref, 4)
    assert entries == 2 * 6 * 4 and float(cnt[:entries].sum()) == 5 * 13 * 21
    C.check_welford_host(slab, cnt, ref, 4, 1e-5)
    absent = next(e for e in range(entries) if C.entry_image_tile(e, 4, 5, 13, 21)[0] >= 5)
    present = next(e for e in range(entries) if C.entry_image_tile(e, 4, 5, 13, 21)[0] == 4)
    bad = slab.clone().view(-1, 64, 2)
    bad[present, 7, 0] += 1e-3                              # one channel of one entry: 5e-7 of the merged mean, 2e-4 of its own
    with pytest.raises(AssertionError):
        C.check_welford_host(bad.reshape(-1), cnt, ref, 4, 1e-5)
    swapped = slab.clone().view(-1, 64, 2)
    swapped[[0, 1]] = swapped[[1, 0]]                       # two images' entries exchanged: every merged figure is unchanged
    with pytest.raises(AssertionError):
        C.check_welford_host(swapped.reshape(-1), cnt, ref, 4, 1e-5)
    c2 = cnt.clone()
    c2[absent] = 64.0
    with pytest.raises(AssertionError, match="counts"):
        C.check_welford_host(slab, c2, ref, 4, 1e-5)
    s2 = slab.clone().view(-1, 64, 2)
    s2[absent, 0, 1] = 1e-9                                 # an absent slot must hold exact zeros
    with pytest.raises(AssertionError):
        C.check_welford_host(s2.reshape(-1), cnt, ref, 4, 1e-5)
    for where in (slab, cnt):
        w2 = where.clone()
        w2[-1] = 0.0                                        # the last guard element
        with pytest.raises(AssertionError, match="out of range"):
            C.check_welford_host(w2 if where is slab else slab, w2 if where is cnt else cnt, ref, 4, 1e-5)
    n2 = slab.clone().view(-1, 64, 2)
    n2[present] = C.NAN
    with pytest.raises(AssertionError, match="not written"):
        C.check_welford_host(n2.reshape(-1), cnt, ref, 4, 1e-5)


def test_check_welford_on_a_single_pixel_asks_for_an_exact_zero_m2():
    ref = torch.randn(1, 128, 1, 1, generator=torch.Generator().manual_seed(7)).double()
    slab, cnt, entries = _welford_slabs(ref, 4)
    assert entries == 4 and cnt[:4].tolist() == [1.0, 0.0, 0.0, 0.0]
    C.check_welford_host(slab, cnt, ref, 4, 1e-5)
    bad = slab.clone().view(-1, 128, 2)
    bad[0, 5, 1] = 1e-12
    with pytest.raises(AssertionError):
        C.check_welford_host(bad.reshape(-1), cnt, ref, 4, 1e-5)


@pytest.mark.parametrize("streamed", [False, True])
def test_check_dgrad_sums_finds_a_wrong_entry_an_absent_slot_and_a_guard_write(streamed):
    g = torch.Generator().manual_seed(6)
    B, H, W = (5, 5, 3) if streamed else (5, 13, 21)
    x, h = torch.randn(B, 128, H, W, generator=g).double(), torch.randn(B, 128, H, W, generator=g).double()
    want = C.streamed_entry_sums(x, h, *C.dgrad1x1_split(B, H, W)) if streamed else C.tiled_entry_sums(x, h, 4)
    assert torch.allclose(want.sum(0)[:, 0], x.sum(dim=(0, 2, 3))) and torch.allclose(want.sum(0)[:, 1], (x * h).sum(dim=(0, 2, 3)))
    slab = torch.cat([want.float(), torch.full((C.GUARD, 128, 2), C.NAN)]).reshape(-1)
    C.check_dgrad_sums_host(slab, want, 1e-4)
    sw = slab.clone().view(-1, 128, 2)
    sw[[0, 1]] = sw[[1, 0]]                                 # the sums over all entries do not see this
    with pytest.raises(AssertionError):
        C.check_dgrad_sums_host(sw.reshape(-1), want, 1e-4)
    if not streamed:
        absent = next(e for e in range(want.shape[0]) if C.entry_image_tile(e, 4, B, H, W)[0] >= B)
        assert float(want[absent].abs().max()) == 0.0
        ab = slab.clone().view(-1, 128, 2)
        ab[absent, 3, 0] = 0.01 * float(want[:, :, 0].abs().max())
        with pytest.raises(AssertionError):
            C.check_dgrad_sums_host(ab.reshape(-1), want, 1e-4)
    gd = slab.clone()
    gd[want.numel()] = 0.0                                  # the first guard element
    with pytest.raises(AssertionError, match="out of range"):
        C.check_dgrad_sums_host(gd, want, 1e-4)


def test_check_tensor_share_is_asserted_from_100_elements_on():
    ref = torch.linspace(1.0, 2.0, 100).double()
    got = C.q16(ref.float())
    C.check_tensor(-1, got, ref)
    off = got.clone()
    off[:2] += 2.0 ** -7                                    # two elements one ulp off: 98 % identical
    with pytest.raises(AssertionError):
        C.check_tensor(-1, off, ref)
    C.check_tensor(-1, off[:64], ref[:64])                  # fewer than 100 elements: the ulp bound alone
    off[0] += 2.0 ** -6
    with pytest.raises(AssertionError):
        C.check_tensor(-1, off[:64], ref[:64])


# ---------------------------------------------------------------------------------------------------------------- honesty
NEW_ROWS = ([("fwd1", r) for r in C.B16K_FWD1_CASES] + [("fwd0", r) for r in C.B16K_FWD0_CASES]
            + [("dgrad", r) for r in C.B16K_DGRAD_CASES] + [("pair", r) for r in C.PAIR_CASES])
SMALL = [("fwd0", (1, 128, 64, 1, 1, 1, True, None, 1, False, 16, 32, 0))]        # 64 outputs: the ulp bound alone


@pytest.mark.parametrize("kind,row", NEW_ROWS, ids=lambda v: C.cid(v) if isinstance(v, tuple) else v)
def test_new_rows_keep_the_gpu_comparison_honest(kind, row):
    """Measured on the reference's own data: the compared tensor has >= 100 elements wherever the 99 % share is asserted (the
    one row below that is listed), it is not degenerate, and in a masked dgrad row at most 1e-4 of the mask pre-activations
    lie within 1e-6 of zero."""
    P = C.make_problem(kind, row)
    ref = P["ref"]
    assert (ref.numel() >= 100) != ((kind, row) in SMALL)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0.1
    assert torch.equal(P["z"], C.q16(P["z"]))
    if P["mz"] is not None:
        assert C.near_zero_share(P) <= 1e-4
        exp, _ = C.dgrad_expected(P, ref.float())
        assert 0.2 < float((exp != 0).double().mean()) < 0.8
    if P["epi"] == 1:
        assert float(ref.var(dim=(0, 2, 3), unbiased=False).min()) > 0 or P["B"] * P["H"] * P["W"] == 1


@pytest.mark.parametrize("key", list(C.BASES))
def test_refusal_bases_keep_the_gpu_comparison_honest(key):
    P = C.base_problem(key)
    assert P["ref"].numel() >= 100
    if P["mz"] is not None:
        assert C.near_zero_share(P) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("key", list(C.BASES))
def test_tsr_conv2d_ex_refuses_every_mutation(key):
    base = C.fake_desc(key)
    muts = C.mutations_of(key)
    assert len(muts) >= 40
    for name, ch in muts:
        st = C.raw_ex(C.mutated(base, ch))
        assert st == 1, f"{key}: tsr_conv2d_ex gave status {st} for: {name}"


def test_the_table_holds_every_refusal_of_the_header_paragraph():
    """include/tactilesr_hip.h, "Refusals" at tsr_conv2d_ex: every branch it lists has a mutation, for every base it concerns."""
    names = {n for n, _, _ in C.MUTATIONS}
    shared = ["d = NULL", "in = NULL", "w_packed = NULL", "out = NULL", "B = 0", "H = -1", "W = 0", "cin = 0", "cin = -16", "cin + 8",
              "in_ctot - 8", "in_coff = 8", "out_ctot - 8", "out_coff = 24", "in_coff = -16", "out_coff = -16",
              "in slice leaves its buffer", "out slice leaves its buffer", "cout = 0", "cout = 32", "cout = 96", "cout = 256",
              "ks = -3", "ks = 0", "ks = 2", "ks = 4", "ks = 7", "epi_mode = -1", "epi_mode = 3", "in_scale without in_shift",
              "in_shift without in_scale", "res_scale without res_shift", "res_shift without res_scale", "nsplit = -5", "nsplit = 4"]
    by_name = {n: keys for n, _, keys in C.MUTATIONS}
    for n in shared:
        assert n in names and set(by_name[n]) == set(C.BASES), n
    for n in ("res_ctot - 8", "res_coff = 8", "res_coff = -16", "res slice leaves its buffer"):
        assert {k for k in C.BASES if k.endswith(("/0", "/2")) and k != "b16k1x1d/2"} == set(by_name[n])
    for n in ("mask_ctot - 8", "mask_coff = 8", "mask_coff = -16", "mask slice leaves its buffer", "epi_mode 2 without mask",
              "bn_a without bn_b", "bn_a without slab"):
        assert {k for k in C.BASES if k.endswith("/2")} == set(by_name[n])
    for n in ("epi_mode 1 without slab", "epi_mode 1 without slab_cnt"):
        assert {k for k in C.BASES if k.endswith("/1")} == set(by_name[n])
    f16 = {"fp16x3/0", "fp16x3/1", "fp16x3/2"}
    assert set(by_name["-2: in_amax = NULL"]) == f16
    bad = [ch["w_inv_scale"] for n, ch, keys in C.MUTATIONS if n.startswith("-2: w_inv_scale") and set(keys) == f16 and ch["w_amax"] is None]
    assert bad[:2] == [0.0, -1.0] and len(bad) == 3 and C.is_nan_value(bad[2])
    assert by_name["-1: 1x1 C_out 64 epi_mode 0, C_in 544 (72 KB of LDS)"] == ("bf16/0",)
    k3 = {"b16k/0", "b16k/1", "b16k/2"}
    for n in ("-3: virtual input, ks > 1", "-3: virtual residual, ks > 1", "-3: C_in 48", "-3: C_in 16", "-3: 8 * in_ctot * H * W >= 2^31"):
        assert set(by_name[n]) == k3
    for n in ("-3: ks = 1, epi_mode 1", "-3: ks = 1, epi_mode 0, plain input", "-3: ks = 1, epi_mode 0, scale", "-3: ks = 1, epi_mode 0, C_in 64"):
        assert by_name[n] == ("b16k1x1f/0",)
    for n in ("-3: ks = 1, epi_mode 2, res", "-3: ks = 1, epi_mode 2, scale", "-3: ks = 1, epi_mode 2, N = 64", "-3: ks = 1, epi_mode 2, K = 128"):
        assert by_name[n] == ("b16k1x1d/2",)
    for n in ("-4: ks = 3", "-4: cout = 64", "-4: epi_mode 0", "-4: epi_mode 2", "-4: no slab", "-4: virtual input", "-4: C_in 48"):
        assert by_name[n] == ("pair/1",)
    assert len(names) == len(C.MUTATIONS)
    assert set(C.CPU_ONLY) <= names
    d = C.fake_desc("b16k/1")
    big = C.mutated(d, by_change("-3: 8 * in_ctot * H * W >= 2^31"))
    assert 8 * big["in_ctot"] * big["H"] * big["W"] >= 2 ** 31
    lds = C.mutated(C.fake_desc("bf16/0"), by_change("-1: 1x1 C_out 64 epi_mode 0, C_in 544 (72 KB of LDS)"))
    assert lds["cin"] * 64 * 2 + lds["cin"] * 8 > 72 * 1024 >= (lds["cin"] - 16) * 136


def by_change(name):
    return next(ch for n, ch, _ in C.MUTATIONS if n == name)
