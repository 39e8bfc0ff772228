"""Kernel-level tests of the fp32 and split-bf16 INFERENCE conv launches, ONE LAUNCH AT A TIME: tsr_conv2d_fwd (`conv_impl =
"f32"`, csrc/conv_mfma_f32.hip), tsr_conv2d_fwd_bf16s with nsplit = 3 / 2 / 1 ("bf16x6" / "bf16x3" / plain bf16 on fp32
tensors, csrc/conv_mfma_split16.hip) and the pack routines that feed them, tsr_pack_conv_weight and tsr_pack_conv_weight_bf16s.

The case tables with the reason and the template instance of every case, the launch geometry, the yardsticks and the bars are
in tests/_infer_f32s.py (checked without a GPU by tests/test_infer_f32s_cpu.py).  In short:

  1. test_*_one_launch over the tables: NaN-filled fp32 buffers 48 channels wider than the slice, input / output / residual at
     three different non-zero offsets, every output element per image -- f32 and x6 against fp64 at TOL = 1e-5; x3 and bf16
     against the fp64 emulation of their plane products at the same TOL, and against the true fp64 at 1e-4 / 2e-2
  2. test_impulse_*, test_delta_*  exact launches, compared with ==: impulses on the borders and tile boundaries ("edge") and
                                   impulses whose whole window lies inside the image ("inner": every packed weight element
                                   exactly once), each with v = 1 and a two-plane v; delta weights on a general input;
                                   together every low-order product
  3. test_pack_*                   the packed weights against their documented layout, bit for bit, the tail of the buffer kept
  4. test_non_finite_*             a NaN / Inf element reaches its ks x ks window of its image and nothing else
  5. refusals                      every mutation of _infer_f32s.mutations / pack_mutations returns 1 and leaves the NaN-filled
                                   output (sentinel-filled pack buffer) as it was; the unmodified list then returns 0 and meets the bar
"""
import functools

import pytest
import torch

import _infer_f32s as S
from _infer_f32s import PAD, TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd  # noqa: F401
    assert torch.cuda.is_available()
    return tactilesr_amd


def dev(t):
    return None if t is None else t.cuda().contiguous()


def stream():
    from tactilesr_amd._lib import stream as st
    return st()


def conv_args(arith, p, offs):
    """Argument list of tsr_conv2d_fwd (arith "f32") / tsr_conv2d_fwd_bf16s (the others) on NaN-padded buffers."""
    x, w = p["x"], p["w"]
    B, cin, H, W = x.shape
    cout, ks = w.shape[0], w.shape[2]
    res = p.get("res")
    a = {"in": S.slice_buffer(x, offs[0]), "in_ctot": cin + PAD, "in_coff": offs[0], "cin": cin, "w_packed": S.pack(arith, w),
         "cout": cout, "ks": ks, "scale": dev(p.get("scale")), "shift": dev(p.get("shift")),
         "res": None if res is None else S.slice_buffer(res, offs[2]), "res_ctot": 0 if res is None else cout + PAD,
         "res_coff": 0 if res is None else offs[2], "out": S.nan_output(B, cout, H, W), "out_ctot": cout + PAD,
         "out_coff": offs[1], "relu": int(p.get("relu", 0)), "B": B, "H": H, "W": W}
    if arith != "f32":
        a["nsplit"] = S.NSPLIT[arith]
    return a


def launch(arith, a):
    st = S.raw(S.KIND[arith], a, stream())
    assert st == 0, f"{S.SIGS[S.KIND[arith]][0]}: status {st}"
    torch.cuda.synchronize()
    return S.read_slice(a["out"], a["B"], a["cout"], a["H"], a["W"], a["out_coff"])[0]


def run(arith, p, offs):
    return launch(arith, conv_args(arith, p, offs))


def held(arith, got, ref, true, tag):
    """The bars of one launch: TOL per image against the yardstick, the project's bar per image against the true fp64."""
    try:
        per = S.check_images(got, ref, TOL)
        per_true = per if true is ref else S.check_images(got, true, S.TRUE_BAR[arith])
    except S.ImageMismatch as e:
        print(f"[{arith}] {tag}: {e}")
        raise
    line = f"[{arith}] {tag}: {S.fmt_images(per)}"
    if true is not ref:
        line += f" of the emulation; true fp64: {S.fmt_images(per_true)}"
    print(line + f"; image max ratio {S.image_ratio(ref):.2f}")
    return per, per_true


# ------------------------------------------------------------------------------------------- 1. one launch at a time
def one_launch(arith, c):
    p, ref, true = S.case_refs(arith, c)
    assert S.image_ratio(ref) < 4
    got = run(arith, p, c.offs)
    held(arith, got, ref, true, f"{S.cid(c)} grid {S.case_grid(arith, c)} {S.instance(arith, c.ks, c.cin, c.cout)}")


@pytest.mark.parametrize("case", S.F32_CASES, ids=S.cid)
def test_f32_one_launch(T, case):
    """tsr_conv2d_fwd: out slice == act(conv(x slice) * scale + shift + res slice) per image against fp64, scale / shift / res
    independently NULL, nothing outside the output slice written."""
    one_launch("f32", case)


@pytest.mark.parametrize("case", S.SPLIT_CASES, ids=S.cid)
@pytest.mark.parametrize("arith", ["x6", "x3"])
def test_split_one_launch(T, arith, case):
    """tsr_conv2d_fwd_bf16s, nsplit 3 (against fp64) and 2 (against its three plane products in fp64, and the true fp64 at 1e-4):
    both halo forms of the 3x3, the weight ring at S = 1 and 2."""
    one_launch(arith, case)


@pytest.mark.parametrize("case", S.BF16_CASES, ids=S.cid)
def test_bf16_one_launch(T, case):
    """tsr_conv2d_fwd_bf16s, nsplit 1: 4 images per workgroup for 3x3 / 5x5, a kernel row (cout 64) or 3 taps (cout 128) per step;
    against conv(bf16 x, bf16 w) in fp64 at TOL and the true fp64 at 2e-2."""
    one_launch("bf16", case)


# ------------------------------------------------------------------------------------------- 2. exact launches
def exact(arith, x, w, tag):
    want = S.exact_ref(arith, x, w)
    got = run(arith, dict(x=x, w=w), S.EXACT_OFFS).double()
    bad = got != want
    n = int(bad.sum())
    if n:
        b, c, y, xx = (int(v) for v in torch.unravel_index(bad.double().argmax(), bad.shape))
        nz = want != 0
        print(f"[{arith}] {tag}: {n} of {want.numel()} elements differ ({int((bad & nz).sum())} of {int(nz.sum())} non-zero ones); first at image "
              f"{b} channel {c} y {y} x {xx}: got {float(got[b, c, y, xx])!r}, want {float(want[b, c, y, xx])!r}")
    assert n == 0, f"{tag}: {n} elements differ"
    return int((want != 0).sum())


@pytest.mark.parametrize("vname", list(S.IMPULSE_V))
@pytest.mark.parametrize("pos", list(S.IMPULSE_POS))
@pytest.mark.parametrize("ks,cin,cout", S.EXACT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("arith", S.ARITHS)
def test_impulse_gives_the_flipped_kernel(T, arith, ks, cin, cout, pos, vname):
    """Image b = one element v of channel b: the output is v times the flipped kernel of channel b around it (f32: rounded once;
    x6: w, and v * w for the two-plane v, bit for bit; x3: its three products; bf16: bf16(w)) and exactly zero elsewhere.  The
    "inner" positions observe all cout * cin * ks * ks weight elements, the "edge" positions what the border leaves."""
    x, w = S.impulse_operands(ks, cin, cout, vname, pos)
    nz = exact(arith, x, w, f"impulse {pos} {vname} {ks}x{ks} {cin}->{cout}")
    assert nz == S.impulse_observed(ks, cin, cout, pos)
    if pos == "inner":
        assert nz == cout * cin * ks * ks


@pytest.mark.parametrize("ks,cin,cout", S.DELTA_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("arith", S.ARITHS)
def test_delta_weight_shifts_the_input(T, arith, ks, cin, cout):
    """w[co, co % cin, co % taps] = 1: output channel co is input channel co % cin shifted by the tap (f32, x6: bit for bit; x3:
    x1 + x2; bf16: bf16(x)), zero where the tap reaches outside the image."""
    x, w = S.delta_operands(ks, cin, cout)
    exact(arith, x, w, f"delta {ks}x{ks} {cin}->{cout}")


# ------------------------------------------------------------------------------------------- 3. pack routines, bit for bit
SENT = 0x7A7A


def bits(t):
    return t.cpu().contiguous().view(torch.int16)


@pytest.mark.parametrize("cout,cin,ks", S.PACK_SHAPES)
def test_pack_conv_weight_layout(T, cout, cin, ks):
    """tsr_pack_conv_weight: element [chunk][tap][kq][co][jj] == w[co][chunk * 16 + kq * 4 + jj][tap], bit for bit."""
    g = torch.Generator().manual_seed(cout + cin + ks)
    w = S.he(g, cout, cin, ks)
    wp = S.pack_f32(w)
    assert wp.numel() == cout * cin * ks * ks
    assert torch.equal(wp.cpu().view(torch.int32), S.pack_f32_layout(w).view(torch.int32))


@pytest.mark.parametrize("ns", [1, 2, 3])
@pytest.mark.parametrize("cout,cin,ks", S.PACK_SHAPES)
def test_pack_conv_weight_bf16s_layout(T, cout, cin, ks, ns):
    """tsr_pack_conv_weight_bf16s into a sentinel-filled buffer of tsr_conv_weight_bf16s_elems: [chunk][step][tap in step][plane][2]
    [co][8] bit for bit, padded tap slots zero, the planes of nsplit 3 sum to w, the tail beyond what the pack writes untouched."""
    from tactilesr_amd._lib import load
    g = torch.Generator().manual_seed(cout + cin + ks)
    w = S.he(g, cout, cin, ks)
    elems = load().tsr_conv_weight_bf16s_elems(cout, cin, ks, ns)
    written = S.bf16s_written(cout, cin, ks, ns)
    assert elems == S.bf16s_elems(cout, cin, ks, ns) >= written
    buf = torch.full((elems,), SENT, dtype=torch.int16, device="cuda")
    assert S.raw("pack_bf16s", dict(w=dev(w), w_packed=buf, cout=cout, cin=cin, ks=ks, nsplit=ns), stream()) == 0
    torch.cuda.synchronize()
    got = buf.cpu()
    want = S.pack_bf16s_layout(w, ns)
    assert want.numel() == written
    assert torch.equal(got[:written], bits(want)), "layout"
    assert bool((got[written:] == SENT).all()), "the pack wrote past nsplit * cout * cin * padded taps"
    nstep, tps = S.tap_slots(ks, cout, ns)
    v = got[:written].view(torch.bfloat16).double().view(cin // 16, nstep * tps, ns, 2, cout, 8)
    assert float(v[:, ks * ks:].abs().max() if nstep * tps > ks * ks else 0.0) == 0, "a padded tap slot is not zero"
    if ns == 3:
        assert torch.equal(v.sum(2)[:, :ks * ks].permute(3, 0, 2, 4, 1).reshape(cout, cin, ks, ks), w.double())
    print(f"[pack bf16s] {cout}x{cin}x{ks}x{ks} nsplit {ns}: {written} written of {elems}, {nstep * tps - ks * ks} padded tap slots")


# ------------------------------------------------------------------------------------------- 4. non-finite input
@functools.lru_cache(maxsize=None)
def nf_refs(arith, ks, cin, cout):
    c = S.nf_case(ks, cin, cout)
    p = S.inputs(c, seed=3)
    return (c, p) + S.yardstick(arith, p)


@pytest.mark.parametrize("bad", [S.NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("ks,cin,cout", S.NF_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("arith", S.ARITHS)
def test_non_finite_input_stays_in_its_receptive_field(T, arith, ks, cin, cout, bad):
    """One non-finite element at (image 1, channel 37, y 7, x 8) of B = 3, 13x21 (scale, shift, residual, no ReLU): the outputs of
    image 1 inside that pixel's ks x ks window are non-finite in every channel; every other output meets the bar of part 1."""
    c, p, ref, true = nf_refs(arith, ks, cin, cout)
    x = p["x"].clone()
    x[1, S.NF_CH, S.NF_Y, S.NF_X] = bad
    got = run(arith, dict(p, x=x), c.offs)
    inside = torch.zeros_like(got, dtype=torch.bool)
    r = ks // 2
    inside[1, :, S.NF_Y - r:S.NF_Y + r + 1, S.NF_X - r:S.NF_X + r + 1] = True
    assert int(inside.sum()) == cout * ks * ks
    assert not torch.isfinite(got[inside]).any(), "a non-finite input did not reach its whole window"
    assert torch.isfinite(got[~inside]).all(), "a non-finite input left its receptive field"
    rest = torch.where(inside, ref.float(), got)
    held(arith, rest, ref, true, f"non-finite {bad} {ks}x{ks} {cin}->{cout}, outside the window")


# ------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("arith", S.ARITHS)
def test_refusals(T, arith):
    """Every mutated argument list returns 1 and launches nothing; the unmodified one returns 0 and meets the bar."""
    c = S.REFUSAL_CASE
    p, ref, true = S.case_refs(arith, c)
    a = conv_args(arith, p, c.offs)
    ints = S.valid_ints(arith)
    assert {k: a[k] for k in ints} == ints, "the GPU test's valid list is the CPU test's"
    kind = S.KIND[arith]
    muts = S.mutations(arith)
    for name, m in muts:
        st = S.raw(kind, dict(a, **m), stream())
        assert st == 1, f"{S.SIGS[kind][0]} with {name}: status {st}"
    torch.cuda.synchronize()
    assert torch.isnan(a["out"]).all(), "a refused call wrote the output"
    got = launch(arith, a)
    held(arith, got, ref, true, f"after {len(muts)} refused argument lists")


@pytest.mark.parametrize("kind", ["pack_f32", "pack_bf16s"])
def test_pack_refusals(T, kind):
    """A refused pack leaves the sentinel-filled buffer as it was; the valid call then writes the documented layout."""
    from tactilesr_amd._lib import load
    ints, muts = S.pack_mutations(kind)
    cout, cin, ks = ints["cout"], ints["cin"], ints["ks"]
    w = S.he(torch.Generator().manual_seed(9), cout, cin, ks)
    elems = 2 * w.numel() if kind == "pack_f32" else load().tsr_conv_weight_bf16s_elems(cout, cin, ks, ints["nsplit"])
    buf = torch.full((elems,), SENT, dtype=torch.int16, device="cuda")
    base = dict(ints, w=dev(w), w_packed=buf)
    for name, m in muts:
        assert S.raw(kind, dict(base, **m), stream()) == 1, f"{S.SIGS[kind][0]} with {name}"
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), f"a refused {S.SIGS[kind][0]} wrote its buffer"
    assert S.raw(kind, base, stream()) == 0
    torch.cuda.synchronize()
    if kind == "pack_f32":
        assert torch.equal(buf.cpu().view(torch.int32), S.pack_f32_layout(w).view(torch.int32))
    else:
        want = bits(S.pack_bf16s_layout(w, ints["nsplit"]))
        assert torch.equal(buf.cpu()[:want.numel()], want) and bool((buf.cpu()[want.numel():] == SENT).all())
    print(f"[refusals] {S.SIGS[kind][0]}: {len(muts)} argument lists refused")
