"""Kernel-level tests of the `tsr_conv2d_ex` launches of the bf16-storage train step that run csrc/conv_b16k.hip and
csrc/conv1x1_b16k.hip (nsplit = -3, and -4 for the stage-1 pair), ONE LAUNCH AT A TIME, and the refusal matrix of
`tsr_conv2d_ex` in every arithmetic.  Tables, references, checkers and the refusal table: tests/_conv_ex_cases.py (its
docstring lists the rows and why; tests/test_conv_ex_cases_cpu.py checks all of it without a device).

1. Every row of the three tables of tests/test_gpu_conv_ex.py, the rows added for these kernels and the pair table run with the
   arithmetic "b16k".  Where `b16k_accepts` says the library takes -3 / -4 the launch runs TWICE on fresh buffers -- input,
   output, residual and mask slices at different offsets of buffers of four different widths, NaN outside every slice and in
   GUARD entries behind the slabs -- and
     * the output meets the bf16-storage bar against fp64 on the bf16-rounded operands (`check_tensor`, ns = -1),
     * epi_mode 1: per-entry counts, per-entry means and the merged mean / variance (TOL[-1]), 4 images per workgroup,
       absent slots exact zeros;
     * epi_mode 2 with bn_a: EVERY entry's sum(x) and sum(x * xhat) (SUM_TOL[-1]; 4 images per workgroup for 3x3 / 5x5, one
       entry per workgroup's contiguous range of 16-pixel groups for the 1x1 kernel) and the sums over all entries;
     * a launch that writes no statistics leaves the slabs' NaN fill alone;
     * out, slab and slab_cnt of the two runs are bit-identical;
     * a virtual input of a 3x3 / 5x5 row is materialised first (tsr_bn_relu_b16, as TrainEngine._plain does) and must equal
       bf16(relu(fma32(z, s, t))) bit for bit.
   Where it says no, the raw call returns status 1 and out, slab and slab_cnt are still all NaN.  `b16k_accepts` itself is
   compared row by row with the library's predicates and the engine's transform rules.
2. Refusals: every base of `_conv_ex_cases.BASES` (one valid launch per arithmetic and epi_mode) returns 0 and the right
   output; every mutation of it returns 1 and leaves out, slab, slab_cnt and out_amax as they were.
"""
import pytest
import torch

import _conv_ex_cases as C
from test_gpu_conv_ex import cb16, nchw, check_outside_untouched, dev, pack_fwd

pytestmark = pytest.mark.gpu

AMAX_SENTINEL = -7.0


@pytest.fixture(scope="module")
def lib():
    import tactilesr_amd                                     # noqa: F401
    from tactilesr_amd._lib import load
    assert torch.cuda.is_available()
    return load()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _accepted(ns, P):
    return C.b16k_accepts(P["kind"], P["row"]) if ns in (C.NS_B16K, C.NS_B16K_PAIR) else True


def _pack(lib, P, ns):
    """The packed weight of problem P for a launch with `ns` (-> tensor, w_amax); a row the library refuses gets a buffer of
    zeros: the pack routines refuse its shape as well."""
    from tactilesr_amd.model._train import _pack_dgrad
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    w = dev(P["w"])
    if not _accepted(ns, P):
        return torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda"), None
    wa = w.abs().max().reshape(1) if ns == -2 else None
    if P["wkind"] == "dgrad":
        return _pack_dgrad(w, w.shape[0], w.shape[1], w.shape[2], P["ci0"], P["cout"], ns, wa), wa
    if ns == C.NS_B16K_PAIR:
        wp = torch.empty(lib.tsr_conv_weight_b16k_pair_elems(P["cin"]), dtype=torch.bfloat16, device="cuda")
        call("tsr_pack_conv_weight_b16k_pair", ptr(w), ptr(wp), I(P["cin"]), stream())
        return wp, None
    if ns == C.NS_B16K:
        wp = torch.empty(lib.tsr_conv_weight_b16k_elems(P["cout"], P["cin"], P["ks"]), dtype=torch.bfloat16, device="cuda")
        call("tsr_pack_conv_weight_b16k", ptr(w), ptr(wp), I(P["cout"]), I(P["cin"]), I(P["ks"]), stream())
        return wp, None
    return pack_fwd(ns, P["w"])


def build(lib, P, ns):
    """The valid descriptor of problem P for a launch with `ns` on fresh NaN-filled device buffers: field -> tensor / int."""
    from tactilesr_amd._lib import call, ptr, stream, c_int as I
    dt = torch.bfloat16 if C.ref_arith(ns) == -1 else torch.float32
    B, H, W, cin, cout, ks = (P[k] for k in ("B", "H", "W", "cin", "cout", "ks"))
    mat = ns in (C.NS_B16K, C.NS_B16K_PAIR) and ks > 1 and P["s"] is not None
    vals, have = C.desc_ints(P, ns, mat), C.desc_ptrs(P, ns, mat)
    zd = cb16(P["z"], cin + C.PADS["in"], P["coff"]["in"], dt)
    s, t = dev(P["s"]), dev(P["t"])
    if mat:
        m = torch.full((B * cin * H * W,), C.NAN, dtype=torch.bfloat16, device="cuda")
        call("tsr_bn_relu_b16", ptr(zd), I(cin + C.PADS["in"]), I(P["coff"]["in"]), I(cin), ptr(s), ptr(t), ptr(m), I(B), I(H * W), stream())
        assert torch.equal(nchw(m, B, cin, H, W), C.materialised(P)), "tsr_bn_relu_b16 is not bf16(relu(fma32(z, s, t)))"
        zd = m
    wp, wa = _pack(lib, P, ns)
    entries = lib.tsr_conv2d_slab_entries_ex(B, H, W, cout, ks, ns)
    T = {"in": zd, "w_packed": wp, "scale": dev(P["scale"]), "shift": dev(P["shift"]), "in_scale": s, "in_shift": t,
         "res_scale": dev(P["rs"]), "res_shift": dev(P["rt"]), "w_amax": wa,
         "slab": torch.full(((entries + C.GUARD) * cout * 2,), C.NAN, device="cuda"),
         "slab_cnt": torch.full((entries + C.GUARD,), C.NAN, device="cuda"),
         "out": torch.full((B * (cout + C.PADS["out"]) * H * W,), C.NAN, dtype=dt, device="cuda"),
         "out_amax": torch.tensor([P["prior"] or 0.0], device="cuda")}
    if P["r"] is not None:
        T["res"] = cb16(P["r"], cout + C.PADS["res"], P["coff"]["res"], dt)
    if P["mz"] is not None:
        T.update(mask=cb16(P["mz"], cout + C.PADS["mask"], P["coff"]["mask"], dt), mask_scale=dev(P["ms"]), mask_shift=dev(P["mh"]),
                 bn_a=dev(P["ba"]), bn_b=dev(P["bb"]))
    if ns == -2:
        T["in_amax"] = torch.tensor([float(P["z"].abs().max())], device="cuda")
    vals.update({k: (T[k] if k in have else None) for k in C.PTR_FIELDS})
    return vals, entries


def launch(vals):
    from tactilesr_amd._lib import stream
    st = C.raw_ex(vals, stream())
    torch.cuda.synchronize()
    return st


def untouched(vals):
    return bool(torch.isnan(vals["out"].float()).all() and torch.isnan(vals["slab"]).all() and torch.isnan(vals["slab_cnt"]).all())


def check(P, ns, vals, entries):
    """Every output of one launch against the fp64 reference of P; returns the figures as text."""
    nsr = C.ref_arith(ns)
    b16k = ns in (C.NS_B16K, C.NS_B16K_PAIR)
    B, H, W, cout, ks = (P[k] for k in ("B", "H", "W", "cout", "ks"))
    oc = P["coff"]["out"]
    full = nchw(vals["out"], B, cout + C.PADS["out"], H, W)
    got = full[:, oc:oc + cout]
    check_outside_untouched(full, oc, cout)
    exp, share = C.dgrad_expected(P, got)
    txt = "out " + C.check_tensor(nsr, got, exp)
    slab, cnt = vals["slab"].cpu(), vals["slab_cnt"].cpu()
    if P["epi"] == 1:
        txt += ", " + C.check_welford_host(slab, cnt, P["ref"], C.images_per_workgroup(ns, ks), C.TOL[nsr])
    elif P["bn"]:
        assert torch.isnan(cnt).all(), "epi_mode 2 wrote slab_cnt"
        if b16k and ks == 1:
            grid, per = C.dgrad1x1_split(B, H, W)
            assert grid == entries
            want = C.streamed_entry_sums(exp, P["xhat"], grid, per)
        else:
            want = C.tiled_entry_sums(exp, P["xhat"], C.images_per_workgroup(ns, ks))
            assert want.shape[0] == entries
        if b16k:
            txt += ", " + C.check_dgrad_sums_host(slab, want, C.SUM_TOL[nsr])
        else:                                               # the other arithmetics' entry order is theirs: the sums over all entries
            sl = slab.double().view(entries + C.GUARD, cout, 2)
            assert torch.isnan(sl[entries:]).all() and torch.isfinite(sl[:entries]).all()
            e = [C.relerr(sl[:entries, :, k].sum(0), want[:, :, k].sum(0)) for k in (0, 1)]
            txt += f", sums {e[0]:.1e} / {e[1]:.1e}"
            assert max(e) < C.SUM_TOL[nsr], txt
        txt += f", near-zero mask share {share:.1e}"
    else:
        assert torch.isnan(slab).all() and torch.isnan(cnt).all(), "a launch without statistics wrote the slabs"
    if vals["out_amax"] is not None:
        assert vals["out_amax"].item() == max(P["prior"] or 0.0, float(got.abs().max()))
    return txt


def _describe(P):
    k = P["kind"]
    if k == "pair":
        return f"pair {P['cin']}->64|64 B={P['B']} {P['H']}x{P['W']} virtual={P['s'] is not None}"
    if k == "dgrad":
        r = P["row"]
        return f"dgrad k{P['ks']} {r[1]}->{r[2]}[{r[4]}:{r[4] + r[3]}] B={P['B']} {P['H']}x{P['W']} {r[9]} res={r[8]} scale={r[10]}"
    return (f"{k} k{P['ks']} {P['cin']}->{P['cout']} B={P['B']} {P['H']}x{P['W']} virtual={P['s'] is not None}"
            + (f" res={P['row'][7]} relu={P['relu']} scale={P['scale'] is not None}" if k == "fwd0" else ""))


ROWS = [(kind, row) for kind, rows in C.TABLES.items() for row in rows]


def _rid(v):
    return C.cid(v) if isinstance(v, tuple) else v


def test_b16k_accepts_agrees_with_the_library(lib):
    """`b16k_accepts` against tsr_conv2d_ex_dgrad_b16k / tsr_conv2d_ex_fwd1x1_b16k plus the rules of TrainEngine (_b16k,
    _res_fwd, _msrb_fwd, _dgrad): a 3x3 / 5x5 input is materialised, a virtual residual keeps a launch off conv_b16k, the 1x1
    forward needs a virtual input and no scale, the 1x1 dgrad a mask and neither res nor scale."""
    dg, f1 = lib.tsr_conv2d_ex_dgrad_b16k, lib.tsr_conv2d_ex_fwd1x1_b16k
    for kind, row in ROWS:
        if kind == "pair":
            want = bool(dg(128, row[0], 5))
        elif kind == "fwd1":
            want = row[0] > 1 and bool(dg(row[2], row[1], row[0]))
        elif kind == "fwd0":
            ks, cin, cout, _, _, _, virt, res, _, use_scale = row[:10]
            want = (bool(dg(cout, cin, ks)) and res != "virtual") if ks > 1 else (virt and not use_scale and bool(f1(cout, cin)))
        else:
            ks, K, _, NP, _, _, _, _, use_res, form, use_scale = row[:11]
            want = bool(dg(NP, K, ks)) and (ks > 1 or (form != "partial" and not use_res and not use_scale))
        assert C.b16k_accepts(kind, row) == want, (kind, row)


@pytest.mark.parametrize("kind,row", ROWS, ids=_rid)
def test_b16k_launch(lib, kind, row):
    ns = C.NS_B16K_PAIR if kind == "pair" else C.NS_B16K
    P = C.make_problem(kind, row)
    vals, entries = build(lib, P, ns)
    st = launch(vals)
    if not C.b16k_accepts(kind, row):
        assert st == 1, f"status {st} for a row conv_b16k cannot run"
        assert untouched(vals), "a refused launch wrote something"
        print(f"[conv_ex b16k] {_describe(P)}: refused")
        return
    assert st == 0
    txt = check(P, ns, vals, entries)
    print(f"[conv_ex b16k] {_describe(P)}: {txt}")
    again, _ = build(lib, P, ns)
    assert launch(again) == 0
    for k in ("out", "slab", "slab_cnt"):
        assert torch.equal(_bits(vals[k]), _bits(again[k])), f"{k} differs between two runs of the same launch"


@pytest.mark.parametrize("key", list(C.BASES))
def test_tsr_conv2d_ex_refusals(lib, key):
    ns = C.BASES[key][0]
    P = C.base_problem(key)
    vals, entries = build(lib, P, ns)
    assert launch(vals) == 0, "the table must mutate a working call"
    print(f"[conv_ex refusals] {key} ({_describe(P)}): {check(P, ns, vals, entries)}")
    vals, _ = build(lib, P, ns)
    if vals["out_amax"] is not None:
        vals["out_amax"].fill_(AMAX_SENTINEL)
    vec = torch.ones(1024, device="cuda")
    buf = torch.zeros(1 << 20, dtype=vals["out"].dtype, device="cuda")
    n = 0
    for name, ch in C.mutations_of(key):
        if name in C.CPU_ONLY:
            continue
        st = launch(C.mutated(vals, ch, vec=vec, buf=buf))
        assert st == 1, f"{key}: status {st} for: {name}"
        assert untouched(vals), f"{key}: wrote something for: {name}"
        assert vals["out_amax"] is None or vals["out_amax"].item() == AMAX_SENTINEL, name
        n += 1
    assert n >= 40
