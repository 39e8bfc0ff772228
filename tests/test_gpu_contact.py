"""GPU checks of the contact readout (tsr_contact_readout, functional.contact_readout / contact_metrics / sr_readout,
eval_func(contact=True)) against the fp64 restatement and THE BARS of tests/_contact_cases.py.  Every output buffer is
prefilled with NaN between NaN guard bands, and every launch runs twice and must give the same bits."""
import math

import numpy as np
import pytest
import torch

import _contact_cases as CC
import _ssim_cases as SC
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib
from tactilesr_amd.train import tactileSR_train as TR

pytestmark = pytest.mark.gpu

NAN, INF = CC.NAN, CC.INF
bits = CC.bits
PI2 = math.pi / 2


def _with_gain(ref, gain):
    out = ref.copy()
    out[:, 2:5] *= gain
    return out


def _pair_gain(pref, ry, rt, gain):
    """The pair and records at `gain` from those at gain 1: masses scale, their relative error does not -- a gain <= 0
    aside, which the tables do not use."""
    return pref, _with_gain(ry, gain), _with_gain(rt, gain)


# ------------------------------------------------------------------------------------------------------------- the kernel
_SHAPE_CASES = [(H, W, B) for (H, W) in CC.SHAPES for B in CC.BATCHES]


@pytest.mark.parametrize("H,W,B", _SHAPE_CASES, ids=[f"{h}x{w}-B{b}" for h, w, b in _SHAPE_CASES])
def test_shapes(H, W, B):
    worst = CC.Worst()
    y, t = CC.shape_images(H, W, B)
    for mode, thr in CC.THRESHOLDS:
        for span in CC.SPANS:
            p1, ry1, rt1 = CC.pair(y, t, mode, thr, 1.0, span)
            for gain in CC.GAINS:
                pref, ry, rt = _pair_gain(p1, ry1, rt1, gain)
                label = (H, W, B, mode, thr, gain, span)
                out = CC.launch(y, t, mode, thr, gain, span)
                CC.check_record(out["rec_y"], ry, span, worst, label + ("y",))
                CC.check_record(out["rec_t"], rt, span, worst, label + ("t",))
                CC.check_pair(out["pair"], pref, ry, rt, span, worst, label)
                single = CC.launch(y, None, mode, thr, gain, span)             # the single form: the pair's own record
                CC.assert_bits(single["rec_y"], out["rec_y"], label + ("single",))
                lone = CC.launch(y, t, mode, thr, gain, span, want=("rec_y", "pair"))    # rec_t is optional
                CC.same_bits(lone, {k: out[k] for k in ("rec_y", "pair")}, label)
    print(worst.line(f"{H}x{W} B={B}"))


def test_grid_cap():
    B, H, W = 2100, 12, 20
    assert B > CC.MAX_WGS
    y, t = CC.blobs(B, H, W, seed=5), CC.blobs(B, H, W, seed=6)
    assert len({r.tobytes() for r in y}) == B                      # distinct images
    worst = CC.Worst()
    for mode, thr in (("abs", 0.3), ("range", 0.5)):
        pref, ry, rt = CC.pair(y, t, mode, thr, 10.0, (4.0, 6.0))
        full = CC.launch(y, t, mode, thr, 10.0, (4.0, 6.0))
        CC.check_record(full["rec_y"], ry, (4.0, 6.0), worst, "cap, y")
        CC.check_record(full["rec_t"], rt, (4.0, 6.0), worst, "cap, t")
        CC.check_pair(full["pair"], pref, ry, rt, (4.0, 6.0), worst, "cap")
        one = CC.launch(y, None, mode, thr, 10.0, (4.0, 6.0))
        for cap in (1, 3):
            CC.same_bits(CC.launch(y, t, mode, thr, 10.0, (4.0, 6.0), max_wgs=cap), full, ("cap", cap))
            CC.same_bits(CC.launch(y, None, mode, thr, 10.0, (4.0, 6.0), max_wgs=cap), one, ("cap, single", cap))
    print(worst.line("2100 images, caps 1 / 3 / default"))


_OFFS = ([(f"{k}+{o}", {k: o}) for k in CC.PTRS for o in (1, 2, 3)] +
         [(f"all+{o}", {k: o for k in CC.PTRS}) for o in (1, 2, 3)] + [("mixed", dict(y=1, t=2, rec_y=3, rec_t=1, pair=2))])


@pytest.mark.parametrize("label,offs", _OFFS, ids=[c[0] for c in _OFFS])
def test_alignment(label, offs):
    y, t = CC.shape_images(40, 40, 7)
    for mode, thr in (("abs", 0.3), ("range", 0.5)):
        base = CC.launch(y, t, mode, thr, 10.0)
        CC.same_bits(CC.launch(y, t, mode, thr, 10.0, offs=offs), base, (label, mode))
        if "y" in offs or "rec_y" in offs:
            single = CC.launch(y, None, mode, thr, 10.0, offs=offs)
            assert torch.equal(bits(single["rec_y"]), bits(base["rec_y"])), (label, mode, "single")


def test_threshold_edges():
    H, W = 8, 12
    span = (4.0, 4.0)
    img = np.zeros((1, H, W), dtype=np.float32)
    img[0, 2, 3:7] = 0.5                                            # exactly tau: excluded
    img[0, 3, 3:6] = 0.75
    img[0, 4, 4] = 1.0
    for mode in ("abs", "range"):                                   # range: mn = 0, mx = 1: tau = 0.5 exactly
        out = CC.launch(img, None, mode, 0.5)["rec_y"]
        CC.check_record(out, CC.record(img, mode, 0.5), span, None, ("tie", mode))
        assert float(out[0, 0]) == 4.0 and float(out[0, 15]) == 0.5, (mode, out[0].tolist())
    out = CC.launch(img, None, "range", 0.0)["rec_y"]               # tau = mn: the minimum's pixels are out
    assert float(out[0, 0]) == 8.0 and float(out[0, 15]) == 0.0
    CC.check_record(out, CC.record(img, "range", 0.0), span, None, "range 0")
    # an all-below image: empty, NaN geometry, entries 0..6 and 15 valid
    out = CC.launch(img, None, "abs", 7.0, 10.0)["rec_y"]
    CC.check_record(out, CC.record(img, "abs", 7.0, 10.0), span, None, "all below")
    assert out[0, :5].tolist() == [0.0, 0.0, 0.0, 10.0 * float(img.sum()), 10.0] and float(out[0, 15]) == 7.0
    assert torch.isnan(out[0, 7:15]).all() and torch.isfinite(out[0, :7]).all()
    # an all-above image
    out = CC.launch(img, None, "abs", -1.0)["rec_y"]
    CC.check_record(out, CC.record(img, "abs", -1.0), span, None, "all above")
    assert float(out[0, 0]) == H * W and abs(float(out[0, 1]) - 16.0) <= 1e-5 * 16 and torch.isfinite(out).all()
    # signed images under a negative abs threshold with sum m v <= 0: a count, no geometry
    neg = np.full((1, H, W), -0.5, dtype=np.float32)
    neg[0, 1, 1:4] = 0.25
    zero = np.zeros((1, H, W), dtype=np.float32)
    zero[0, 2, 2], zero[0, 5, 9] = 1.0, -1.0                        # sum m v == 0 exactly
    for im, n in ((neg, H * W), (zero, H * W)):
        out = CC.launch(im, None, "abs", -2.0)["rec_y"]
        CC.check_record(out, CC.record(im, "abs", -2.0), span, None, "signed")
        assert float(out[0, 0]) == n and torch.isnan(out[0, 7:15]).all() and torch.isfinite(out[0, :7]).all()
    signed = CC.blobs(7, 40, 40, seed=3, signed=True)               # and signed blobs with a contact
    assert (signed < 0).any()
    for thr in (-0.125, 0.25):
        assert CC.margin_ok(signed, "abs", thr)
        CC.check_record(CC.launch(signed, None, "abs", thr)["rec_y"], CC.record(signed, "abs", thr), span, None, ("signed", thr))


@pytest.mark.parametrize("H,W,points,first", [
    (40, 40, [(39, 39), (20, 3), (5, 17)], (5, 17)),
    (5, 7, [(4, 6), (4, 5), (2, 0)], (2, 0)),
    (8, 8, [(3, 5), (3, 6), (3, 7)], (3, 5)),                       # inside one quad
    (160, 160, [(7, 80), (0, 40)], (0, 40)),                        # index 1200 (thread 44) after index 40 (thread 10)
    (160, 160, [(6, 64), (6, 60)], (6, 60)),                        # index 1024 (thread 0, second round) after 1020 (thread 255)
    (160, 160, [(159, 159), (80, 80), (80, 79)], (80, 79)),
])
def test_peak_ties_take_the_first_maximum_in_row_major_order(H, W, points, first):
    img = CC.quantise(0.25 * np.random.default_rng(H).random((1, H, W)))
    for x, c in points:
        img[0, x, c] = 1.5
    for off in (0, 1):                                              # both load paths
        out = CC.launch(img, None, "abs", 0.5, offs=dict(y=off))["rec_y"]
        CC.check_record(out, CC.record(img, "abs", 0.5), (4.0, 4.0), None, ("ties", off))
        want = ((first[0] + 0.5) * 4 / H - 0.5, (first[1] + 0.5) * 4 / W - 0.5)
        assert abs(float(out[0, 5]) - want[0]) <= 4e-5 and abs(float(out[0, 6]) - want[1]) <= 4e-5, (out[0, 5:7], want)
        assert float(out[0, 0]) == len(points) and float(out[0, 4]) == 1.5


@pytest.mark.parametrize("H,W", [(40, 40), (5, 7), (100, 100)])
def test_one_pixel_contact(H, W):
    span = (4.0, 6.0)
    for x, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        img = CC.impulses(H, W, [(x, c, 0.7001953125)])
        for mode, thr in (("abs", 0.0), ("range", 0.5), ("abs", 0.3)):
            out = CC.launch(img, None, mode, thr, 10.0, span)["rec_y"]
            CC.check_record(out, CC.record(img, mode, thr, 10.0, span), span, None, ("one pixel", x, c, mode))
            assert not torch.isnan(out).any() and float(out[0, 0]) == 1.0
            want = ((x + 0.5) * span[0] / H - 0.5, (c + 0.5) * span[1] / W - 0.5)
            assert abs(float(out[0, 7]) - want[0]) <= 1e-5 * span[0] and abs(float(out[0, 8]) - want[1]) <= 1e-5 * span[1]
            assert (out[0, 9:15] == 0).all(), out[0, 9:15].tolist()         # moments, angle, axes: exactly 0


def test_rectangle_and_impulse_closed_forms():
    span = (4.0, 4.0)
    for H, W, r0, r1, c0, c1 in ((40, 40, 5, 17, 10, 16), (40, 40, 20, 24, 3, 30), (100, 100, 30, 31, 10, 90), (5, 7, 1, 4, 2, 7)):
        img = CC.rectangle(H, W, r0, r1, c0, c1, 0.75)
        out = CC.launch(img, None, "abs", 0.0, 1.0, span)["rec_y"]
        CC.check_record(out, CC.record(img, "abs", 0.0, 1.0, span), span, None, "rectangle")
        pr, pc, nr, nc = span[0] / H, span[1] / W, r1 - r0, c1 - c0
        want = [(r0 + r1) / 2 * pr - 0.5, (c0 + c1) / 2 * pc - 0.5, (nr * nr - 1) / 12 * pr * pr, (nc * nc - 1) / 12 * pc * pc, 0.0]
        got = out[0, 7:12].double().tolist()
        for g, w, s in zip(got, want, (4, 4, 16, 16, 16)):
            assert abs(g - w) <= 1e-5 * s, (got, want)
        th = abs(float(out[0, 12]))
        assert min(th, abs(PI2 - th)) <= 1e-5 and (th < 1) == (want[2] > want[3]), (th, want)
        assert float(out[0, 0]) == nr * nc and abs(float(out[0, 2]) - 0.75 * nr * nc) <= 1e-5 * 0.75 * nr * nc
    for H, W, a, b in ((40, 40, (10, 10), (20, 20)), (40, 40, (10, 30), (30, 10)), (100, 100, (5, 50), (80, 50)),
                       (40, 40, (7, 3), (7, 33)), (5, 7, (0, 1), (3, 6)), (40, 40, (3, 4), (13, 33))):
        for sp in ((4.0, 4.0), (4.0, 6.0)):
            img = CC.impulses(H, W, [a + (0.5,), b + (0.5,)])
            out = CC.launch(img, None, "abs", 0.25, 1.0, sp)["rec_y"]
            CC.check_record(out, CC.record(img, "abs", 0.25, 1.0, sp), sp, None, "two impulses")
            du, dv = (b[0] - a[0]) * sp[0] / H, (b[1] - a[1]) * sp[1] / W
            want = math.atan2(dv, du)
            want = want - math.pi if want > PI2 else want + math.pi if want <= -PI2 else want
            d = abs(float(out[0, 12]) - want)
            assert min(d, math.pi - d) <= 1e-5, (a, b, sp, float(out[0, 12]), want)
            assert abs(float(out[0, 13]) - math.hypot(du, dv) / 2) <= 1e-5 * min(sp) and abs(float(out[0, 14])) <= 1e-5 * min(sp)


@pytest.mark.parametrize("n", [40, 100])
def test_a_block_over_a_taxel_has_its_centroid_at_the_taxel(n):
    q = n // 4
    imgs = np.concatenate([CC.rectangle(n, n, a * q, (a + 1) * q, c * q, (c + 1) * q, 1.0 + 0.25 * a + 0.0625 * c)
                           for a in range(4) for c in range(4)])
    out = CC.launch(imgs, None, "range", 0.5)["rec_y"]
    CC.check_record(out, CC.record(imgs, "range", 0.5), (4.0, 4.0), None, "taxel blocks")
    want = torch.tensor([[a, c] for a in range(4) for c in range(4)], dtype=torch.float64)
    assert float((out[:, 7:9].double() - want).abs().max()) <= 4e-5
    assert float((out[:, 1].double() - 1.0).abs().max()) <= 1e-5   # one square pitch
    if n == 100:                                                    # the reference's mask centres: pixel 12 + 25 a is u = a
        pts = CC.impulses(100, 100, [(12 + 25 * 2, 12 + 25 * 3, 1.0)])
        got = CC.launch(pts, None, "abs", 0.0)["rec_y"][0, 5:9].tolist()
        assert got == [2.0, 3.0, 2.0, 3.0], got


def test_pair_cases():
    span = (4.0, 4.0)
    y, t = CC.shape_images(40, 40, 7)
    for tt in (y, y.copy()):                                        # one buffer twice, and an equal copy
        out = CC.launch(y, tt, "abs", 0.3, 10.0)
        assert torch.equal(bits(out["rec_y"]), bits(out["rec_t"]))
        p = out["pair"]
        assert (p[:, 2] == 1).all() and (p[:, 3] == 1).all() and (p[:, 4] == 0).all() and (p[:, 5] == 0).all()
        assert (p[:, 6] == 0).all() and (p[:, 7] == 0).all() and torch.equal(p[:, 0], p[:, 1]) and torch.equal(p[:, 0], out["rec_y"][:, 0])
    a, b = CC.rectangle(40, 40, 2, 10, 2, 10), CC.rectangle(40, 40, 20, 30, 25, 35)
    empty = np.zeros((1, 40, 40), dtype=np.float32)
    cases = {"disjoint": (a, b), "both empty": (empty, empty.copy()), "y empty": (empty, b), "t empty": (a, empty),
             "nested": (CC.rectangle(40, 40, 2, 12, 2, 12), a), "overlap": (a, CC.rectangle(40, 40, 6, 16, 6, 12, 2.0))}
    for name, (yy, tt) in cases.items():
        out = CC.launch(yy, tt, "abs", 0.5)
        pref, ry, rt = CC.pair(yy, tt, "abs", 0.5)
        CC.check_record(out["rec_y"], ry, span, None, name)
        CC.check_record(out["rec_t"], rt, span, None, name)
        CC.check_pair(out["pair"], pref, ry, rt, span, None, name)
        p = out["pair"][0].tolist()
        if name == "disjoint":
            assert p[0] == 0 and p[1] == 164 and p[2] == 0 and p[3] == 0 and p[4] > 1
        elif name == "both empty":
            assert p[:4] == [0, 0, 1, 1] and math.isnan(p[4]) and math.isnan(p[5]) and math.isnan(p[7]) and p[6] == 0
        elif name == "y empty":
            assert p[2] == 0 and math.isnan(p[4]) and p[5] == 1 and math.isnan(p[7])
        elif name == "t empty":
            assert p[2] == 0 and math.isnan(p[4]) and math.isnan(p[5]) and math.isnan(p[7])
        elif name == "nested":
            assert p[0] == 64 and p[1] == 100 and abs(p[2] - 0.64) <= 1e-5 and abs(p[3] - 128 / 164) <= 1e-5


@pytest.mark.parametrize("where", ["y", "t", "both"])
def test_non_finite_inputs_stay_in_their_own_image(where):
    B, H, W = 600, 12, 20
    y, t = CC.blobs(B, H, W, seed=21), CC.blobs(B, H, W, seed=22)
    clean = CC.launch(y, t, "range", 0.5, 10.0)
    assert torch.isfinite(clean["rec_y"][:, :7]).all() and torch.isfinite(clean["pair"][:, :4]).all()
    bad = list(range(7, 600, 37))[:16]
    assert len(bad) == 16
    yb, tb = y.copy(), t.copy()
    vals = (NAN, INF, -INF, NAN)
    for n, i in enumerate(bad):
        pos = ((n * 5) % H, (n * 7) % W) if n else (H - 1, W - 1)
        if where in ("y", "both"):
            yb[i][pos] = vals[n % 4]
        if where in ("t", "both"):
            tb[i][pos[0], (pos[1] + 3) % W] = vals[(n + 1) % 4]
    out = CC.launch(yb, tb, "range", 0.5, 10.0)
    keep = torch.ones(B, dtype=torch.bool)
    keep[bad] = False
    for k in out:
        assert torch.equal(bits(out[k][keep]), bits(clean[k][keep])), (k, "a clean image changed")
    for i in bad:
        assert torch.isnan(out["pair"][i]).all(), i
        for k, hit in (("rec_y", where in ("y", "both")), ("rec_t", where in ("t", "both"))):
            if hit:
                assert torch.isnan(out[k][i]).all(), (k, i)
            else:                                                   # the clean partner keeps its own record
                assert torch.equal(bits(out[k][i]), bits(clean[k][i])), (k, i)
    pref, ry, rt = CC.pair(yb, tb, "range", 0.5, 10.0)             # and the restatement agrees on the pattern
    CC.check_record(out["rec_y"], ry, (4.0, 4.0), None, "non-finite y")
    CC.check_record(out["rec_t"], rt, (4.0, 4.0), None, "non-finite t")
    CC.check_pair(out["pair"], pref, ry, rt, (4.0, 4.0), None, "non-finite")
    if where == "y":                                                # the single form, and an image that is all NaN
        yb[bad[0]] = NAN
        one = CC.launch(yb, None, "abs", 0.3)["rec_y"]
        ref = CC.launch(y, None, "abs", 0.3)["rec_y"]
        assert torch.equal(bits(one[keep]), bits(ref[keep])) and torch.isnan(one[bad]).all()


def _refusal_call(a):
    B, H, W = max(a["B"], 1), 8, 8
    y = torch.rand(B * H * W + 64, device="cuda")
    t = torch.rand(B * H * W + 64, device="cuda")
    bufs = {k: CC.placed(n) for k, n in (("rec_y", CC.REC * B), ("rec_t", CC.REC * B), ("pair", CC.PAIR * B))}
    addr = dict(y=y.data_ptr(), t=t.data_ptr(), **{k: v[1].data_ptr() for k, v in bufs.items()})
    keep = (y.clone(), t.clone())
    st = CC.call_raw(_lib.load(), a, stream=torch.cuda.current_stream().cuda_stream, **CC.resolve_ptrs(a, addr))
    torch.cuda.synchronize()
    return st, bufs, torch.equal(y, keep[0]) and torch.equal(t, keep[1])


@pytest.mark.parametrize("label,over", CC.REFUSALS, ids=[r[0] for r in CC.REFUSALS])
def test_refusal_matrix(label, over):
    a = dict(CC.BASE_ARGS, **over)
    if a["H"] > 8 or a["W"] > 8:                                    # the refused size is never allocated
        assert CC.call_raw(_lib.load(), a, y=1 << 20, t=1 << 30, rec_y=1 << 40, rec_t=1 << 41, pair=1 << 42) == 1
        return
    st, bufs, inputs_kept = _refusal_call(a)
    assert st == 1, (label, st)
    assert all(torch.isnan(b[0]).all() for b in bufs.values()) and inputs_kept, (label, "a refused call wrote")


@pytest.mark.parametrize("label,over", CC.ACCEPTED, ids=[r[0] for r in CC.ACCEPTED])
def test_the_table_refuses_no_more_than_the_header(label, over):
    a = dict(CC.BASE_ARGS, **over)
    st, bufs, inputs_kept = _refusal_call(a)
    assert st == 0 and inputs_kept, (label, st)
    for k, (buf, mid, start) in bufs.items():
        assert bool(torch.isnan(mid[:1]).any()) != bool(a[k]) or k == "pair", (label, k)      # written where given
        assert CC.guards_intact(buf, start, mid.numel()), (label, k)


def test_graph_capture_replays_on_rewritten_inputs():
    sets = [CC.shape_images(40, 40, 7), CC.shape_images(40, 40, 7)[::-1], (CC.blobs(7, 40, 40, 91), CC.blobs(7, 40, 40, 92))]
    y = torch.from_numpy(sets[0][0])[:, None].cuda().contiguous()
    t = torch.from_numpy(sets[0][1])[:, None].cuda().contiguous()
    kw = dict(threshold=0.5, mode="range", gain=10.0, span=(4.0, 6.0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Fh.contact_metrics(y, t, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        met, ry, rt = Fh.contact_metrics(y, t, **kw)
    seen = []
    for a, b in sets:
        y.copy_(torch.from_numpy(a)[:, None])
        t.copy_(torch.from_numpy(b)[:, None])
        graph.replay()
        seen.append((met.raw.clone(), ry.raw.clone(), rt.raw.clone()))
    torch.cuda.synchronize()
    for (a, b), got in zip(sets, seen):
        em, ey, et = Fh.contact_metrics(torch.from_numpy(a)[:, None].cuda(), torch.from_numpy(b)[:, None].cuda(), **kw)
        for g, e in zip(got, (em.raw, ey.raw, et.raw)):
            assert torch.equal(bits(g), bits(e))
        pref, r1, r2 = CC.pair(a, b, "range", 0.5, 10.0, (4.0, 6.0))
        CC.check_pair(got[0].cpu(), pref, r1, r2, (4.0, 6.0), None, "graph")
    assert not torch.equal(seen[0][0], seen[2][0])


# ------------------------------------------------------------------------------------------------------ functional layer
def test_functional_forms():
    y, t = CC.shape_images(40, 40, 7)
    yd, td = torch.from_numpy(y).cuda(), torch.from_numpy(t).cuda()       # (B,H,W)
    raw = CC.launch(y, t, "abs", 0.3, 10.0, (4.0, 6.0))
    r = Fh.contact_readout(yd, 0.3, "abs", 10.0, (4.0, 6.0))
    assert isinstance(r, Fh.ContactReadout) and r.raw.shape == (7, 16) and r.raw.is_cuda
    assert torch.equal(bits(r.raw.cpu()), bits(raw["rec_y"]))
    for name, cols in (("count", 0), ("area", 1), ("mass", 2), ("total", 3), ("peak", 4), ("peak_pos", slice(5, 7)),
                       ("centroid", slice(7, 9)), ("moments", slice(9, 12)), ("angle", 12), ("major", 13), ("minor", 14),
                       ("tau", 15)):
        f = getattr(r, name)
        assert torch.equal(f, r.raw[:, cols]) and f.shape == ((7,) if isinstance(cols, int) else (7, cols.stop - cols.start))
    r4 = Fh.contact_readout(yd[:, None], 0.3, "abs", 10.0, (4.0, 6.0), max_wgs=2)            # (B,1,H,W), a grid cap
    assert torch.equal(bits(r4.raw), bits(r.raw))
    m, ry, rt = Fh.contact_metrics(yd, td[:, None], 0.3, "abs", 10.0, (4.0, 6.0))
    assert isinstance(m, Fh.ContactMetrics) and m.raw.shape == (7, 8)
    assert torch.equal(bits(m.raw.cpu()), bits(raw["pair"])) and torch.equal(bits(ry.raw.cpu()), bits(raw["rec_y"]))
    assert torch.equal(bits(rt.raw.cpu()), bits(raw["rec_t"]))
    for i, name in enumerate(("inter", "union", "iou", "dice", "centroid_dist", "mass_rel_err", "peak_dist", "angle_diff")):
        assert torch.equal(getattr(m, name), m.raw[:, i])
    nc = yd[:, ::2]                                                 # a non-contiguous view is made contiguous
    assert torch.equal(bits(Fh.contact_readout(nc).raw.cpu()), bits(CC.launch(np.ascontiguousarray(y[:, ::2]), None, "abs", 0.0)["rec_y"]))
    one = Fh.contact_readout(yd, span=3.0)                          # one number: a square span
    assert torch.equal(bits(one.raw), bits(Fh.contact_readout(yd, span=(3.0, 3.0)).raw))
    for bad in (dict(mode="rel"), dict(threshold=NAN), dict(mode="range", threshold=1.0), dict(gain=INF), dict(span=(4.0, 0.0)),
                dict(span=(1, 2, 3)), dict(max_wgs=0), dict(threshold="x")):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.contact_readout(yd, **bad)
    for bad in (yd.double(), yd[0], yd[:, None].expand(-1, 2, -1, -1), yd.cpu()):
        with pytest.raises(_lib.TactileSRHipError):
            Fh.contact_readout(bad)
    with pytest.raises(_lib.TactileSRHipError):
        Fh.contact_metrics(yd, td[:3])
    with pytest.raises(_lib.TactileSRHipError):
        Fh.contact_metrics(yd, td.cpu())
    assert not r.raw.requires_grad and not Fh.contact_readout(yd.clone().requires_grad_(True)).raw.requires_grad


# ------------------------------------------------------------------------------------------------------------ end to end
def _model(seed=42):
    torch.manual_seed(seed)
    return tactilesr_amd.TactileSR(10, 1, 3, 1, 1).cuda().eval()


def _batch(B, seed):
    """Random taxels and a contact-like HR: blobs of amplitude <= 100 raw, <= 10 after HR_scale_num."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (SC.blobs(B, 100, 100, g) * 10).cuda()


def test_sr_readout_is_the_forward_and_the_launch():
    m = _model()
    m.train()
    LR, _ = _batch(4, 5)
    kw = dict(threshold=0.5, mode="range", gain=10.0)
    out, r = Fh.sr_readout(m, LR, **kw)
    assert m.training and not out.requires_grad and out.shape == (4, 1, 40, 40)
    m.eval()
    with torch.no_grad():
        assert torch.equal(out, m(LR))
    ref = CC.record(out[:, 0].cpu().numpy(), "range", 0.5, 10.0)
    assert (ref[:, 0] > 0).all()
    CC.check_record(r.raw.cpu(), ref, (4.0, 4.0), None, "sr_readout")
    assert torch.equal(bits(r.raw), bits(Fh.contact_readout(out, **kw).raw))
    ran = []
    m.register_forward_pre_hook(lambda *a: ran.append(1))
    with pytest.raises(_lib.TactileSRHipError):                     # a bad keyword raises before the forward
        Fh.sr_readout(m, LR, mode="rel")
    assert not ran


def _set_means(model, loader, conf, weights=None):
    """The restatement's whole-set means of (IoU, centroid distance, relative mass error)."""
    thr, mode, gain, span = TR.contact_readout_config(conf)
    rows, ws = [], []
    with torch.no_grad():
        for i, b in enumerate(loader):
            LR, HR = TR._prep(b, conf, "cuda")
            out = model(LR)
            rows.append(CC.pair(out[:, 0].cpu().numpy(), HR[:, 0].cpu().numpy(), mode, thr, gain, span)[0][:, [2, 4, 5]])
            ws.append(np.ones(len(rows[-1])) if weights is None else weights[i].double().numpy())
    v, w = np.concatenate(rows), np.concatenate(ws)
    out = []
    for j in range(3):
        keep = ~np.isnan(v[:, j]) & (w != 0)
        out.append(float((w[keep] * v[keep, j]).sum() / w[keep].sum()) if keep.any() else NAN)
    return out, v


@pytest.mark.parametrize("bs", [8, 3])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_eval_func_contact_scores(bs, weighted):
    m = _model()
    conf = dict(TR.default_config(), contact_threshold=0.25, contact_span=(4, 6))
    loader = [_batch(bs, 31 + i) for i in range(3)]
    loader[1][1][1] = 0.0                                           # a target without contact: NaN distance and mass error
    weights = None
    if weighted:
        g = torch.Generator().manual_seed(3)
        weights = [torch.rand(bs, generator=g) + 0.25 for _ in loader]
        weights[0][0] = 0.0                                         # an unlabeled sample
        loader = [(b[0], b[1], None, w.cuda()) for b, w in zip(loader, weights)]
    base = TR.eval_func(m, loader, conf)
    got = TR.eval_func(m, loader, conf, contact=True)
    assert len(base) == 3 and len(got) == 6 and tuple(got[:3]) == tuple(base)             # the leading values: the same bits
    both = TR.eval_func(m, loader, dict(conf, degradation_gamma=0.7), windowed_ssim=True, degradation=True, contact=True)
    assert len(both) == 8 and tuple(both[:3]) == tuple(base) and tuple(both[5:]) == tuple(got[3:])
    want, v = _set_means(m, loader, conf, weights)
    assert np.isnan(v[:, 1]).sum() >= 1 and (~np.isnan(v[:, 1])).sum() >= bs          # some left out, most counted
    for g_, w_, s in zip(got[3:], want, (1.0, 4.0, 1.0)):
        assert abs(g_ - w_) <= 1e-5 * max(s, abs(w_)), (got[3:], want)
    rng = TR.eval_func(m, loader, dict(conf, contact_threshold=0.5, contact_threshold_mode="range"), contact=True)
    want_r, _ = _set_means(m, loader, dict(conf, contact_threshold=0.5, contact_threshold_mode="range"), weights)
    for g_, w_, s in zip(rng[3:], want_r, (1.0, 4.0, 1.0)):
        assert abs(g_ - w_) <= 1e-5 * max(s, abs(w_)), (rng[3:], want_r)
    if not weighted:                                                # composes with the ensemble and the noise
        ens = TR.eval_func(m, loader, conf, self_ensemble="rot90", taxel_noise=dict(sigma_add=0.02), contact=True)
        plain = TR.eval_func(m, loader, conf, self_ensemble="rot90", taxel_noise=dict(sigma_add=0.02))
        assert len(ens) == 6 and tuple(ens[:3]) == tuple(plain) and all(math.isfinite(x) for x in ens[3:])
        none = TR.eval_func(m, loader, dict(conf, contact_threshold=1e6), contact=True)     # no contact anywhere
        assert none[3] == 1.0 and math.isnan(none[4]) and math.isnan(none[5])
