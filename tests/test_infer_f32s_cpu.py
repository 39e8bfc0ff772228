"""CPU checks of tests/_infer_f32s.py and of the host-side argument checks of tsr_conv2d_fwd, tsr_conv2d_fwd_bf16s,
tsr_pack_conv_weight and tsr_pack_conv_weight_bf16s.

  * The case tables are well formed, hold the shapes and grids they are meant to, and -- with the exact launches -- reach each
    of the 28 inference instances.
  * The emulated references (x3, bf16) are the plane products they claim to be and sit inside the project's bars against the
    true fp64 on their own.
  * The expected tensors of the exact launches equal an fp32 emulation in the kernel's product order, and every one of the three
    low-order products of bf16x6 is seen by at least one of them.
  * The pack restatements and the `_elems` arithmetic.
  * Refusals: every mutation comes back as status exactly 1.  The pointers are fake (never dereferenced); an argument list that
    is NOT refused reaches a launch, which without a device comes back as status 2.
"""
import re

import pytest
import torch
import torch.nn.functional as F

import _infer_f32s as S
from _infer_f32s import PAD, FAKE, TOL


# ------------------------------------------------------------------------------------------------------- case tables
def _shapes(cases):
    return {(c.ks, c.cin, c.cout, c.B, c.H, c.W) for c in cases}


def test_the_issue_s_shapes_are_all_there():
    assert _shapes(S.F32_CASES) == {(3, 64, 64, 3, 40, 40), (5, 128, 128, 2, 13, 21), (1, 16, 64, 1, 1, 1), (1, 32, 128, 5, 9, 17),
                                    (3, 16, 128, 1, 5, 3), (5, 48, 64, 2, 1, 1), (5, 16, 64, 1, 3, 5), (1, 256, 64, 70, 12, 12),
                                    (3, 128, 64, 64, 12, 12), (5, 64, 128, 3, 40, 40), (3, 448, 64, 1, 8, 8)}
    assert _shapes(S.SPLIT_CASES) == {(3, 64, 64, 3, 40, 40), (3, 48, 128, 5, 13, 21), (3, 32, 128, 1, 5, 3), (3, 16, 64, 2, 1, 1),
                                      (3, 448, 64, 1, 8, 8), (3, 128, 64, 64, 12, 12), (5, 128, 128, 2, 13, 21), (5, 48, 64, 3, 5, 3),
                                      (5, 16, 128, 1, 3, 5), (5, 64, 64, 3, 40, 40), (1, 16, 64, 1, 1, 1), (1, 32, 128, 5, 9, 17),
                                      (1, 256, 64, 70, 12, 12)}
    assert _shapes(S.BF16_CASES) == {(3, 64, 64, 5, 40, 40), (3, 16, 128, 1, 1, 1), (5, 48, 128, 2, 5, 3), (5, 128, 64, 6, 13, 21),
                                     (5, 64, 128, 3, 40, 40), (5, 16, 64, 1, 3, 5), (3, 128, 64, 74, 12, 12), (3, 128, 128, 64, 12, 12),
                                     (3, 448, 64, 1, 8, 8), (1, 16, 64, 1, 1, 1), (1, 32, 128, 3, 13, 21), (1, 256, 64, 70, 12, 12)}
    assert len(S.F32_CASES) == 11 and len(S.SPLIT_CASES) == 13 and len(S.BF16_CASES) == 12


@pytest.mark.parametrize("name", list(S.TABLES))
def test_case_table_is_well_formed(name):
    cases = S.TABLES[name]
    for c in cases:
        assert len(set(c.offs)) == 3 and set(c.offs) == {16, 32, 48}, "three different non-zero offsets"
        for width, ctot, coff in S.case_slices(c):
            assert width % 16 == 0 and ctot % 16 == 0 and coff % 16 == 0 and ctot == width + PAD
            assert 0 < coff and coff + width <= ctot
        assert c.H <= 40 and c.W <= 40 and c.B <= 74 and c.B * c.H * c.W <= 74 * 12 * 12, "nothing larger than 40x40 or B = 74 at 12x12"
        assert c.ks in (1, 3, 5) and c.cout in (64, 128) and c.cin % 16 == 0
    assert {(c.scale, c.shift) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}
    assert {(c.res, c.relu) for c in cases} == {(True, 1), (True, 0), (False, 1), (False, 0)}
    assert {c.offs[0] for c in cases} == {16, 32, 48} and len({c.offs for c in cases}) == 6, "the offsets rotate"
    assert any(c.H == 1 and c.W == 1 for c in cases) and any(c.H < 8 and c.W < 8 and c.H * c.W > 1 for c in cases)
    assert any(c.H % 8 and c.W % 8 and c.H > 8 for c in cases), "ragged on both axes"


def test_grids_follow_the_launchers():
    want = {"f32": [50, 6, 1, 18, 1, 1, 1, 140, 128, 50, 1], "split": [50, 18, 1, 1, 1, 128, 6, 2, 1, 50, 1, 18, 140],
            "bf16": [50, 1, 1, 12, 25, 1, 76, 64, 1, 1, 12, 140]}
    for name, grids in want.items():
        for a in S.TABLE_ARITHS[name]:
            assert [S.case_grid(a, c) for c in S.TABLES[name]] == grids, (name, a)
    assert 140 % 8 == 4 and 76 % 8 == 4 and 128 % 8 == 0 and 64 % 8 == 0
    assert S.images_per_workgroup("bf16", 1) == 2 and S.images_per_workgroup("bf16", 5) == 4 and S.images_per_workgroup("x3", 3) == 2


def test_tap_slots_and_slab_items():
    """The padded tap slots and DMA pass shapes the docstring of _infer_f32s states."""
    assert [S.tap_slots(ks, co, 3) for ks in (1, 3, 5) for co in (64, 128)] == [(1, 1), (1, 1), (9, 1), (9, 1), (25, 1), (25, 1)]
    assert [S.tap_slots(ks, co, 2) for ks in (1, 3, 5) for co in (64, 128)] == [(1, 1), (1, 1), (5, 2), (5, 2), (13, 2), (13, 2)]
    assert [S.tap_slots(ks, co, 1) for ks in (1, 3, 5) for co in (64, 128)] == [(1, 1), (1, 1), (3, 3), (3, 3), (5, 5), (9, 3)]
    assert 5 * 2 == 10 and 13 * 2 == 26 and 9 * 3 == 27          # x3: 10 / 26 slots, bf16 5x5 x 128: 27 slots, two of them zero
    assert S.slab_items(3, 64, 3) == 384 and S.slab_items(3, 128, 3) == 768 and S.slab_items(1, 64, 3) == 384
    assert S.slab_items(1, 64, 1) == 128 and S.slab_items(1, 128, 1) == 256 and S.slab_items(5, 64, 1) == 640
    assert S.slab_items(3, 64, 2) == 512 and S.slab_items(1, 64, 2) == 256
    # a partial DMA pass (items % 256 != 0) is reached by part 1 and part 2 in every arithmetic that has one
    for a in ("x6", "bf16"):
        tab = S.SPLIT_CASES if a == "x6" else S.BF16_CASES
        assert any(S.slab_items(c.ks, c.cout, S.NSPLIT[a]) % 256 for c in tab)
        assert any(S.slab_items(ks, cout, S.NSPLIT[a]) % 256 for ks, _, cout in S.EXACT_SHAPES)
    assert {S.slab_items(c.ks, c.cout, 1) for c in S.BF16_CASES} >= {128, 256, 384, 640, 768}


def test_the_step_counts_the_tables_name():
    by = {(c.ks, c.cin, c.cout): S.steps("f32", c.ks, c.cin, c.cout) for c in S.F32_CASES}
    assert by[(1, 16, 64)] == 1 and by[(1, 32, 128)] == 2 and by[(3, 448, 64)] == 28 * 9
    for a in ("x6", "x3"):
        by = {(c.ks, c.cin, c.cout): S.steps(a, c.ks, c.cin, c.cout) for c in S.SPLIT_CASES}
        assert by[(1, 16, 64)] == 1 and by[(1, 32, 128)] == 2
    by = {(c.ks, c.cin, c.cout): S.steps("bf16", c.ks, c.cin, c.cout) for c in S.BF16_CASES}
    assert by[(1, 16, 64)] == 1 and by[(1, 32, 128)] == 2 and by[(3, 16, 128)] == 3 and by[(5, 48, 128)] == 27
    # double-buffered halo: one pair, two pairs, 14 pairs; the single-buffer 3x3 form with one and with three blocks
    forms = {(c.cin // 16, S.instance("x6", c.ks, c.cin, c.cout)[3]) for c in S.SPLIT_CASES if c.ks == 3}
    assert forms >= {(2, "dbh"), (4, "dbh"), (28, "dbh"), (1, "single"), (3, "single")}


def test_every_instance_is_launched_by_part_1_and_by_part_2():
    every = set(S.all_instances())
    assert len(every) == 28 and len([i for i in every if i[0] == "f32"]) == 6 and len([i for i in every if i[0] == "bf16"]) == 6
    assert len([i for i in every if i[0] == "x6"]) == 8 and len([i for i in every if i[0] == "x3"]) == 8
    part1 = {S.instance(a, c.ks, c.cin, c.cout) for name, cases in S.TABLES.items() for a in S.TABLE_ARITHS[name] for c in cases}
    part2 = {S.instance(a, ks, cin, cout) for a in S.ARITHS for ks, cin, cout in S.EXACT_SHAPES}
    assert part1 == every and part2 == every
    assert len(S.EXACT_SHAPES) == 8 and {(ks, cout) for ks, cin, cout in S.EXACT_SHAPES if cin == 32} == {(k, c) for k in (1, 3, 5) for c in (64, 128)}
    assert set(S.DELTA_SHAPES) == {(3, 32, 128), (5, 32, 128), (1, 64, 64)} and (S.DELTA_B, S.DELTA_H, S.DELTA_W) == (3, 13, 21)


@pytest.mark.parametrize("name", list(S.TABLES))
def test_images_of_a_case_have_one_magnitude_and_the_emulation_is_inside_the_project_bars(name):
    """max_b max|ref_b| / min_b max|ref_b| < 4 for every case (the per-image bar is the tensor-wide bar up to that factor), and
    the emulated references alone meet 1e-4 (x3) / 2e-2 (bf16) per image against the true fp64 -- by a margin that leaves room
    for the device's TOL."""
    worst = {}
    for a in S.TABLE_ARITHS[name]:
        for c in S.TABLES[name]:
            p, ref, true = S.case_refs(a, c)
            assert torch.isfinite(ref).all() and S.image_ratio(ref) < 4 and S.image_ratio(true) < 4, (a, c, S.image_ratio(ref))
            if a in ("x3", "bf16"):
                per = S.check_images(ref, true, S.TRUE_BAR[a] - TOL * 1.01)
                worst[a] = max(worst.get(a, 0.0), float(per.max()))
                assert float(per.max()) > 0, "the emulation is not the true convolution"
    print(name, {a: f"{v:.2e}" for a, v in worst.items()})


# ------------------------------------------------------------------------------------------------------- references
def test_planes_are_the_bf16_split():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(4096, generator=g) * 3
    p = S.planes(v, 3)
    assert torch.equal(p[0], v.bfloat16().float()) and torch.equal(p[1], (v - p[0]).bfloat16().float())
    assert torch.equal(p[0].double() + p[1].double() + p[2].double(), v.double()), "three planes hold an fp32 value exactly"
    assert all(torch.equal(q, q.bfloat16().float()) for q in p)
    assert torch.equal(S.planes(v, 2)[1], p[1]) and torch.equal(S.planes(v, 1)[0], p[0])
    assert not torch.equal(p[0] + p[1], v)
    one = S.planes(torch.tensor([1.0 + 2.0 ** -8]), 3)
    assert [float(q) for q in one] == [1.0, 2.0 ** -8, 0.0]
    w14 = S.round14(v)
    q = S.planes(w14, 3)
    assert float(q[2].abs().max()) == 0 and torch.equal(q[0] + q[1], w14) and float(((w14 - v) / v).abs().max()) <= 2.0 ** -14
    assert bool((w14.view(torch.int32) & 1023 == 0).all())


def test_ref_emulated_is_the_sum_of_its_products():
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(2, 32, 9, 11, generator=g) * 3, torch.randn(64, 32, 5, 5, generator=g) * 0.1
    s, t, r = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g), torch.randn(2, 64, 9, 11, generator=g)
    x1, x2 = S.planes(x, 2)
    w1, w2 = S.planes(w, 2)
    c = lambda a, b: F.conv2d(a.double(), b.double(), padding=2)                # noqa: E731
    want = c(x1, w1) + c(x1, w2) + c(x2, w1)
    assert torch.allclose(S.ref_emulated("x3", x, w), want, rtol=1e-13, atol=1e-13)
    assert torch.allclose(S.plane_conv("x3", x, w), want, rtol=1e-13, atol=1e-13)
    assert torch.equal(S.ref_emulated("bf16", x, w), c(x1, w1))
    ep = F.relu(want * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1) + r.double())
    assert torch.allclose(S.ref_emulated("x3", x, w, s, t, r, 1), ep, rtol=1e-13, atol=1e-13)
    assert torch.allclose(S.ref_emulated("x3", x, w, None, t, None, 0), want + t.double().view(1, -1, 1, 1), rtol=1e-13, atol=1e-13)
    # the dropped product x2w2 is what separates x3 from the true convolution: ~2^-16
    true = c(x, w)
    e3 = float((want - true).abs().max() / true.abs().max())
    e1 = float((c(x1, w1) - true).abs().max() / true.abs().max())
    assert 1e-7 < e3 < 1e-4 and 1e-4 < e1 < 2e-2
    x6 = S.plane_conv("x6", x, w)
    assert float((x6 - true).abs().max() / true.abs().max()) < 1e-6
    p = dict(x=x, w=w, scale=s, shift=None, res=r, relu=1)
    y6 = S.yardstick("x6", p)
    assert y6[0] is y6[1] and torch.equal(S.yardstick("f32", p)[0], S.ref_conv(x, w, s, None, r, 1))
    assert torch.equal(S.yardstick("x3", p)[0], S.ref_emulated("x3", x, w, s, None, r, 1))


def _c_int(expr, ns):
    """Value of a C integer expression made of literals, parentheses and `NS == n ? a : b` for NS = ns."""
    e = expr.strip()
    while e.startswith("("):                       # strip parentheses that enclose the whole expression
        depth = 0
        for i, ch in enumerate(e):
            depth += (ch == "(") - (ch == ")")
            if depth == 0:
                break
        if i != len(e) - 1:
            break
        e = e[1:-1].strip()
    depth, q = 0, -1
    for i, ch in enumerate(e):
        depth += (ch == "(") - (ch == ")")
        if ch == "?" and depth == 0:
            q = i
            break
    if q < 0:
        return int(e)
    depth, nested = 0, 0
    for i in range(q + 1, len(e)):
        ch = e[i]
        depth += (ch == "(") - (ch == ")")
        if depth == 0 and ch == "?":
            nested += 1
        if depth == 0 and ch == ":":
            if nested == 0:
                break
            nested -= 1
    m = re.fullmatch(r"NS\s*==\s*(\d+)", e[:q].strip())
    assert m, e
    return _c_int(e[q + 1:i], ns) if ns == int(m.group(1)) else _c_int(e[i + 1:], ns)


def _top_level_split(body):
    out, depth, cur = [], 0, ""
    for ch in body:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return out + [cur]


def test_the_products_are_the_kernel_s():
    """PRODUCTS against the kernel's own text: the PA / PB arrays and NPROD parsed out of csrc/conv_mfma_split16.hip, of which
    the MFMA loop takes the entries 6 - NPROD + q, q = 0 .. NPROD - 1."""
    from tactilesr_amd import _lib
    with open(_lib.os.path.join(_lib._HERE, "csrc", "conv_mfma_split16.hip")) as f:
        src = f.read()
    arr = {n: re.search(r"constexpr int %s\[6\] = \{(.*?)\};" % n, src).group(1) for n in ("PA", "PB")}
    nprod = re.search(r"constexpr int NPROD = (.*?);", src).group(1)
    assert "fa[cur][PA[6 - NPROD + q]][mb], fb[cur][PB[6 - NPROD + q]][nb]" in src and "for (int q = 0; q < NPROD; ++q)" in src

    def pa_pb(ns):
        pa = [_c_int(e, ns) for e in _top_level_split(arr["PA"])]
        pb = [_c_int(e, ns) for e in _top_level_split(arr["PB"])]
        n = _c_int(nprod, ns)
        assert len(pa) == len(pb) == 6 and n == {3: 6, 2: 3, 1: 1}[ns]
        return list(zip(pa, pb))[6 - n:]
    assert S.PRODUCTS["x6"] == pa_pb(3) and S.PRODUCTS["x3"] == pa_pb(2) and S.PRODUCTS["bf16"] == pa_pb(1)
    assert set(S.PRODUCTS["x6"]) == {(a, b) for a in range(3) for b in range(3) if a + b <= 2}


# ------------------------------------------------------------------------------------------------------- exact launches
def _flipped_kernel(x, w, v, ks, pos):
    """The impulse response written out: out[b, :, py - kh + P, px - kw + P] = v * w[:, b, kh, kw] inside the image."""
    B, P = x.shape[0], ks // 2
    out = torch.zeros(B, w.shape[0], S.IMPULSE_H, S.IMPULSE_W, dtype=torch.float64)
    for b in range(B):
        py, px = S.IMPULSE_POS[pos][b % 16]
        for kh in range(ks):
            for kw in range(ks):
                y, xx = py - kh + P, px - kw + P
                if 0 <= y < S.IMPULSE_H and 0 <= xx < S.IMPULSE_W:
                    out[b, :, y, xx] = v * w[:, b, kh, kw].double()
    return out


def test_impulse_positions():
    assert set(S.IMPULSE_POS) == {"edge", "inner"}
    pos = set(S.IMPULSE_POS["edge"])
    assert len(pos) == 16 and all(0 <= y < S.IMPULSE_H and 0 <= x < S.IMPULSE_W for y, x in pos)
    assert pos >= {(0, 0), (0, 9), (8, 0), (8, 9)}, "the four corners"
    assert pos >= {(7, 7), (7, 8), (8, 7), (8, 8)} and {y for y, _ in pos} >= {7, 8} and {x for _, x in pos} >= {7, 8}
    assert -(-S.IMPULSE_H // 8) == 2 and -(-S.IMPULSE_W // 8) == 2
    inner = set(S.IMPULSE_POS["inner"])
    assert len(inner) == 16 and all(2 <= y <= S.IMPULSE_H - 3 and 2 <= x <= S.IMPULSE_W - 3 for y, x in inner), "a whole 5x5 window inside"
    assert any(y == 6 for y, _ in inner) and any(x >= 6 for _, x in inner), "3x3 windows that straddle the tile boundary at 7 | 8"
    assert any(y >= 6 and x >= 6 for y, x in inner), "a window over all four tiles"
    for name in S.IMPULSE_POS:
        x = S.impulse_input(32, 1.5, name)
        assert x.shape == (32, 32, 9, 10) and int((x != 0).sum()) == 32 and all(float(x[b, b].abs().max()) == 1.5 for b in range(32))


def test_what_the_impulse_launches_observe():
    """"inner": every weight element once.  "edge": what the border leaves -- 1x1 all, 3x3 71.5 %, 5x5 60.3 %."""
    for ks, cin, cout in S.EXACT_SHAPES:
        assert S.impulse_observed(ks, cin, cout, "inner") == cout * cin * ks * ks
    assert S.impulse_observed(1, 32, 64, "edge") == 64 * 32
    assert S.impulse_observed(3, 32, 64, "edge") == 13184 and S.impulse_observed(5, 32, 64, "edge") == 30848
    assert S.impulse_observed(3, 48, 128, "edge") == 128 * 48 * 9 * 13184 // 18432


@pytest.mark.parametrize("ks,cin,cout", S.EXACT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("pos", list(S.IMPULSE_POS))
def test_impulse_expectations(ks, cin, cout, pos):
    for vname, v in S.IMPULSE_V.items():
        x, w = S.impulse_operands(ks, cin, cout, vname, pos)
        assert x.shape[0] == cin and float(x.max()) == v and float(w.abs().min()) > 0
        w1, w2, w3 = S.planes(w, 3)
        for a in S.ARITHS:
            want = S.exact_ref(a, x, w)
            assert torch.equal(want, want.float().double()), "the expectation is an fp32 value"
            assert torch.equal(S.exact_emulated_f32(a, x, w).double(), want), (a, vname)
            weff = {("f32", "one"): w.double(), ("x6", "one"): w.double(), ("x3", "one"): w1.double() + w2.double(),
                    ("bf16", "one"): w1.double(), ("bf16", "split"): w1.double(),
                    ("f32", "split"): (w.double() * v).float().double(), ("x6", "split"): w.double() * v,
                    ("x3", "split"): w.double() + 2.0 ** -8 * w1.double()}[(a, vname)]
            assert torch.equal(want, _flipped_kernel(x, weff, 1.0, ks, pos)), (a, vname)
            assert int((want != 0).sum()) == S.impulse_observed(ks, cin, cout, pos), "every observed element gives a non-zero output"
            if pos == "inner":                      # each (co, ci, tap) exactly once: the flipped window holds the whole kernel
                P = ks // 2
                for b in (0, cin // 2 + 1, cin - 1):
                    py, px = S.IMPULSE_POS[pos][b % 16]
                    win = want[b, :, py - P:py + P + 1, px - P:px + P + 1].flip(1, 2)
                    assert torch.equal(win, weff[:, b]), (a, vname, b)
        if vname == "split":
            assert float(w3.abs().max()) == 0 and torch.equal(w1 + w2, w)
        else:
            assert float((w3 != 0).float().mean()) > 0.9


@pytest.mark.parametrize("ks,cin,cout", S.DELTA_SHAPES, ids=lambda v: str(v))
def test_delta_expectations(ks, cin, cout):
    x, w = S.delta_operands(ks, cin, cout)
    assert int((w != 0).sum()) == cout and torch.equal(w.sum(dim=(1, 2, 3)), torch.ones(cout))
    hit = w.view(cout, cin, ks * ks).sum(0)
    assert bool((hit.sum(1) > 0).all()) and bool((hit.sum(0) > 0).all()), "every input channel and every tap is used"
    x1, x2, x3 = S.planes(x, 3)
    P = ks // 2
    for a in S.ARITHS:
        want = S.exact_ref(a, x, w)
        assert torch.equal(S.exact_emulated_f32(a, x, w).double(), want), a
        src = {"f32": x.double(), "x6": x.double(), "x3": x1.double() + x2.double(), "bf16": x1.double()}[a]
        pad = F.pad(src, (P, P, P, P))
        for co in range(cout):
            ci, tap = co % cin, co % (ks * ks)
            kh, kw = tap // ks, tap % ks
            assert torch.equal(want[:, co], pad[:, ci, kh:kh + S.DELTA_H, kw:kw + S.DELTA_W]), (a, co)
    assert float((x3 != 0).float().mean()) > 0.9


def test_every_low_order_product_is_seen():
    """x3w1, x1w3, x2w2 -- the three products a 1e-5 bar cannot see: dropping any one changes the expectation of at least one
    exact launch (and 98 % of the elements where it does)."""
    full = S.PRODUCTS["x6"]
    launches = [("impulse one",) + S.impulse_operands(3, 32, 64, "one", "inner"), ("impulse split",) + S.impulse_operands(3, 32, 64, "split", "inner"),
                ("delta",) + S.delta_operands(3, 32, 128)]
    seen = {}
    for drop in [(2, 0), (0, 2), (1, 1)]:
        mutant = [p for p in full if p != drop]
        assert len(mutant) == 5
        for name, x, w in launches:
            want = S.exact_ref("x6", x, w)
            got = S.exact_ref("x6", x, w, mutant)
            nz = want != 0
            share = float((got != want)[nz].float().mean())
            if share > 0:
                seen.setdefault(drop, []).append((name, share))
    assert set(seen) == {(2, 0), (0, 2), (1, 1)}, seen
    assert dict(seen[(1, 1)])["impulse split"] > 0.9 and dict(seen[(0, 2)])["impulse one"] > 0.9 and dict(seen[(2, 0)])["delta"] > 0.9
    # on the "inner" set that is a share of ALL weight elements: x1w3 is observed on every element with w3 != 0, x2w2 on every
    # element with w2 != 0 (the delta launches observe x3w1 on every input element with x3 != 0)
    for vname, drop in (("one", (0, 2)), ("split", (1, 1))):
        x, w = S.impulse_operands(5, 32, 128, vname, "inner")
        changed = S.exact_ref("x6", x, w, [p for p in full if p != drop]) != S.exact_ref("x6", x, w)
        plane = S.planes(w, 3)[drop[1]]
        assert int(changed.sum()) == int((plane != 0).sum()) > 0.9 * w.numel(), (vname, drop)
    # and what each costs against the true value is below what a 1e-5 bar can see
    p = S.inputs(S.Case(3, 64, 64, 2, 13, 21, False, False, False, 0, (16, 32, 48)))
    x, w = p["x"], p["w"]
    true = S.conv64(x, w)
    for drop in [(2, 0), (0, 2), (1, 1)]:
        e = float((S.plane_conv("x6", x, w, [p for p in full if p != drop]) - true).abs().max() / true.abs().max())
        assert 1e-7 < e < TOL, (drop, e)


# ------------------------------------------------------------------------------------------------------- packs
def test_pack_layout_restatements():
    g = torch.Generator().manual_seed(5)
    for cout, cin, ks in S.PACK_SHAPES:
        w = S.he(g, cout, cin, ks)
        T = ks * ks
        wp = S.pack_f32_layout(w).view(cin // 16, T, 4, cout, 4)
        for chunk, tap, kq, n, jj in [(0, 0, 0, 0, 0), (cin // 16 - 1, T - 1, 3, cout - 1, 3), (0, T // 2, 2, 17, 1)]:
            assert wp[chunk, tap, kq, n, jj] == w.view(cout, cin, T)[n, chunk * 16 + kq * 4 + jj, tap]
        assert torch.equal(wp.reshape(-1).sort().values, w.reshape(-1).sort().values)
        for ns in (1, 2, 3):
            nstep, tps = S.tap_slots(ks, cout, ns)
            TP = nstep * tps
            q = S.pack_bf16s_layout(w, ns)
            assert q.dtype == torch.bfloat16 and q.numel() == S.bf16s_written(cout, cin, ks, ns) == ns * cout * cin * TP
            q = q.float().view(cin // 16, TP, ns, 2, cout, 8)
            pl = S.planes(w, ns)
            for chunk, tap, p, kh, n, j in [(0, 0, 0, 0, 0, 0), (cin // 16 - 1, T - 1, ns - 1, 1, cout - 1, 7), (0, T // 2, 0, 1, 17, 3)]:
                assert q[chunk, tap, p, kh, n, j] == pl[p].view(cout, cin, T)[n, chunk * 16 + kh * 8 + j, tap]
            assert float(q[:, T:].abs().max() if TP > T else 0.0) == 0, "padded tap slots are zero"
            if ns == 3:
                assert torch.equal(q.double().sum(2)[:, :T].permute(3, 0, 2, 4, 1).reshape(cout, cin, T), w.double().view(cout, cin, T))


def test_packed_weight_sizes():
    from tactilesr_amd._lib import load
    lib = load()
    tails = 0
    for cout, cin, ks in S.PACK_SHAPES + [(64, 448, 3), (128, 128, 5)]:
        for ns in (1, 2, 3):
            n = lib.tsr_conv_weight_bf16s_elems(cout, cin, ks, ns)
            assert n == S.bf16s_elems(cout, cin, ks, ns) >= S.bf16s_written(cout, cin, ks, ns)
            tails += n > S.bf16s_written(cout, cin, ks, ns)
    assert S.bf16s_elems(64, 16, 1, 3) == 2 * S.bf16s_written(64, 16, 1, 3), "the K = 32 bound: one block padded to a pair"
    assert S.bf16s_elems(128, 48, 5, 2) == 2 * 128 * 64 * 25 > S.bf16s_written(128, 48, 5, 2) == 2 * 128 * 48 * 26
    assert S.bf16s_elems(64, 32, 3, 2) == S.bf16s_written(64, 32, 3, 2) == 2 * 64 * 32 * 10
    assert tails >= 6


# ------------------------------------------------------------------------------------------------------- refusals
def fake_list(arith):
    v = S.valid_ints(arith)
    v.update({p: FAKE for p in S.POINTERS})
    return v


@pytest.mark.parametrize("arith", S.ARITHS)
def test_every_mutation_is_refused(arith):
    base = fake_list(arith)
    muts = S.mutations(arith)
    assert len({n for n, _ in muts}) == len(muts)
    for name, m in muts:
        assert all(k in base for k in m), (name, m)
        assert S.raw(S.KIND[arith], dict(base, **m)) == 1, f"{S.SIGS[S.KIND[arith]][0]} accepted: {name}"
    # a NULL scale / shift / res is no refusal, and an unused residual's slice arguments are not looked at
    if not torch.cuda.is_available():           # without a device the valid list passes every check and fails at the launch
        assert S.raw(S.KIND[arith], base) == 2
        for p in ("scale", "shift", "res"):
            assert S.raw(S.KIND[arith], dict(base, **{p: None})) == 2
        assert S.raw(S.KIND[arith], dict(base, res=None, res_ctot=0, res_coff=-16)) == 2


def test_the_tables_hold_the_refusals_the_header_lists():
    for a in S.ARITHS:
        names = {n for n, _ in S.mutations(a)}
        want = {"NULL in", "NULL w_packed", "NULL out", "B = 0", "B = -1", "H = 0", "H = -1", "W = 0", "W = -1", "cin = 0",
                "cin negative", "cin + 8", "in_ctot - 8", "in_coff 8", "out_ctot - 8", "out_coff 24", "res_ctot - 8", "res_coff 8",
                "in_coff negative", "out_coff negative", "res_coff negative", "in slice past the end", "out slice past the end",
                "res slice past the end", "cout = 0", "cout = 32", "cout = 96", "cout = 256", "ks = 0", "ks = 2", "ks = 4", "ks = 7"}
        if a != "f32":
            want |= {"nsplit = 0", "nsplit = 4", "nsplit = -1"}
        assert want <= names, (a, want - names)
    c = S.REFUSAL_CASE
    assert c.scale and c.shift and c.res and set(c.offs) == {16, 32, 48}


@pytest.mark.parametrize("kind", ["pack_f32", "pack_bf16s"])
def test_pack_routines_refuse(kind):
    ints, muts = S.pack_mutations(kind)
    base = dict(ints, w=FAKE, w_packed=FAKE)
    names = {n for n, _ in muts}
    assert {"NULL w", "NULL w_packed", "cin = 0", "cin negative", "cin + 8", "cout = 32", "ks = 2"} <= names
    for name, m in muts:
        assert S.raw(kind, dict(base, **m)) == 1, f"{S.SIGS[kind][0]} accepted: {name}"
    if not torch.cuda.is_available():
        assert S.raw(kind, base) == 2
        if kind == "pack_bf16s":
            assert all(S.raw(kind, dict(base, nsplit=n)) == 2 for n in (1, 2, 3))


def test_abi_and_header():
    from tactilesr_amd import _lib
    assert _lib.ABI_VERSION == 24 and _lib.load().tsr_abi_version() == 24
    with open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "tactilesr_hip.h")) as f:
        header = f.read()
    assert "Refusals (status 1, nothing is launched, `out` is untouched) of tsr_conv2d_fwd and tsr_conv2d_fwd_bf16s" in header
