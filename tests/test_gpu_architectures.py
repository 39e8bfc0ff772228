"""TactileSR across stem counts and block counts (case tables and reasons: tests/_arch_cases.py; their CPU preconditions:
tests/test_arch_cases_cpu.py).  The kernel tests cover every launch on its own; what varies here is the ARCHITECTURE that
strings the launches together: seqsCnt 1 .. 10 (the fuse conv, its data and weight gradients at C_in 192 .. 640 inside a
model, with per-stem channel offsets, per-frame taxel gradients and max|.| slots), zero MSRBs / ResBlocks (the copy paths of
the eval forward), several ResBlocks (the ping-pong of the force branch, the block loops of the train engine), and the
dominance cases d1 .. d3, in which the copied half of the head's input is far above the other half: the fp16x3 head conv needs
an upper bound of max|input|, and a copy has no epilogue that raises it (d1 .. d3 fail in fp16x3 without the two
`torch.maximum` of `TactileSR._infer_pass`).

Everything at scale_factor 3, B = 3 (train: the B of `_arch_cases.TRAIN_B`), against the fp64 oracle.

Bars: eval TOL = 1e-5 of the output maximum (e5 / e6: max(1e-5, 4 * e_ref), `_arch_cases.eval_bar`; e_ref, the error of
torch's fp32 CPU forward against fp64, is 6.5e-07 / 1.1e-06 as measured by tests/test_arch_cases_cpu.py, so both are 1e-5); train: the bars of
`_gradcheck.train_step_vs_oracle` at tol = 1e-5, and the ReLU-flip cap of `_gradcheck.check_pattern`; bf16 storage: the
helpers' own bars.

Worst figure per case and arithmetic as measured on an MI355X (max-norm error of the image / worst on-pattern gradient error):
    eval          fp16x3   f32      bf16x6  |               fp16x3   f32      bf16x6
      e1          2.3e-06  3.2e-06  3.8e-06 |   e8          2.3e-06  2.3e-06  2.9e-06
      e2          1.7e-06  2.3e-06  2.2e-06 |   e9          1.4e-06  2.3e-06  2.7e-06
      e3          3.9e-06  3.8e-06  3.4e-06 |   e10         2.3e-06  3.1e-06  3.1e-06
      e4          1.8e-06  1.2e-06  1.8e-06 |   d1          7.9e-07  9.4e-07  1.2e-06
      e5          1.8e-06  1.8e-06  2.0e-06 |   d2          1.2e-06  1.4e-06  1.5e-06
      e6          2.3e-06  3.4e-06  3.5e-06 |   d3          1.8e-06  1.1e-06  1.4e-06
      e7          1.3e-06  1.7e-06  1.4e-06 |   unfused fp16x3: e1 2.0e-06, e6 2.3e-06
    stages (worst stage, fp16x3 / f32 / bf16x6): e4 2.0e-06 / 1.9e-06 / 3.0e-06; e10 1.1e-06 / 1.1e-06 / 1.7e-06
    train (worst on-pattern gradient): fp16x3 t1 3.5e-06 (B 1) 4.5e-06 (B 3), t2 4.9e-06, t3 4.4e-06 / 4.4e-06, t4 6.5e-06,
      t5 5.2e-06; f32 t1 4.2e-06 / 5.5e-06, t5 5.0e-06; bf16x6 t1 6.7e-06 / 7.2e-06, t5 6.5e-06
    taxel gradient: t1 2.2e-06 / 2.7e-06, t3 2.4e-06 / 2.6e-06;  bf16 train worst cosine: t1 0.99993 / 0.99561, t3 0.99821 / 0.99860
    bf16 eval, teacher-forced differing share / beyond one ulp; end-to-end rel-L2: e1 4.1e-03 / 3.3e-04; 6.9e-03,
      e2 3.4e-03 / 7.2e-05; 1.2e-03, e3 6.7e-03 / 4.3e-04; 9.5e-03, e4 3.6e-04 / 0; 2.0e-03 (block by block), e5 1.7e-03 / 0; 3.1e-03, e6 2.2e-03 / 1.8e-04; 8.3e-03

On the code before the two `torch.maximum` of `_infer_pass`, d1, d2 and d3 each returned a wholly non-finite image in fp16x3
(432 of 432 pixels; f32 and bf16x6 passed), and all six train-refusal cases found advanced running statistics.

Two things the first hardware run taught:
  * With the lattice seeds e2 and e3 were the worst-conditioned networks of the table (e_ref 3.6e-06 / 5.5e-06; e2's image
    maximum 2.2): e2 gave fp16x3 1.01e-05 and bf16x6 1.32e-05 against 1e-5 (f32 passed), e3 f32 9.2e-06 and, in bf16, an end-to-end
    rel-L2 of 3.9e-02 against 3e-2.  The cases now carry the CPU condition 4 * e_ref <= 1e-5 and seeds that meet it
    (tests/_arch_cases.py); the bars are unchanged.
  * e4 in bf16 through the helper as it was: teacher-forced "force" differing share 6.8e-02 (bar 1e-2), beyond one ulp 8.0e-03
    (bar 1e-3) at max-norm 3.7e-03 -- the oracle has no teacher point between ResBlocks, so three of them ran un-forced.
    `bf16_eval_vs_emulating_oracle` now restates the force branch block by block on the device's "res{i}" stages.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O
import _arch_cases as A
import _gradcheck as GC

pytestmark = pytest.mark.gpu

IMPLS = ["fp16x3", "f32", "bf16x6"]


@pytest.fixture(scope="module")
def T():
    import tactilesr_amd  # noqa: F401
    from tactilesr_amd.model import tactileSR_model as M
    assert torch.cuda.is_available()
    return M


def _eval_model(T, cid, impl, **attrs):
    cfg, sd, LR, _ = A.case_data(cid)
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.conv_impl = impl
    for k, v in attrs.items():
        setattr(m, k, v)
    return m, LR.cuda()


def _check_image(tag, y, cid):
    ref = A.eval_ref(cid)[0]
    assert y.shape == (A.B, 1, 4 * A.SF, 4 * A.SF)
    finite = bool(torch.isfinite(y).all())
    e = GC.relerr(y, ref) if finite else float("inf")
    print(f"[arch {tag}] {e:.1e}" + ("" if finite else f" ({int((~torch.isfinite(y)).sum())} non-finite pixels)"))
    assert finite and e < A.eval_bar(cid), (e, A.eval_bar(cid))
    return e


# ------------------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("cid", A.EVAL_IDS)
def test_eval_forward_vs_fp64_oracle(T, cid, impl):
    m, LR = _eval_model(T, cid, impl)
    _check_image(f"{cid} {impl}", m(LR), cid)


@pytest.mark.parametrize("cid", ["e1", "e6"])
def test_eval_forward_unfused_vs_fp64_oracle(T, cid):
    """fp16x3 with the stage-1 pair and the fused 1x1 off: the separate launches of every MSRB."""
    m, LR = _eval_model(T, cid, "fp16x3", fuse_pair=False, fuse_1x1=False)
    _check_image(f"{cid} fp16x3 unfused", m(LR), cid)


@pytest.mark.parametrize("cid", A.FULL)
def test_eval_forward_bf16_storage_vs_bf16_emulating_oracle(T, cid):
    cfg, sd, LR, _ = A.case_data(cid)
    r = GC.bf16_eval_vs_emulating_oracle(T, cfg, sd, LR)
    print(f"[arch {cid} bf16] teacher-forced differing {r[0]:.2e}, beyond one ulp {r[1]:.2e}, max-norm {r[2]:.2e}, "
          f"rel-L2 {r[3]:.2e}; end-to-end rel-L2 {r[4]:.2e}, max {r[5]:.2e}")


@pytest.mark.parametrize("cid", A.COPY)
def test_eval_forward_bf16_storage_without_a_block_is_refused(T, cid):
    from tactilesr_amd import _lib
    m, LR = _eval_model(T, cid, "bf16")
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with pytest.raises(_lib.TactileSRHipError, match="needs at least one MSRB and one ResBlock"):
        m(LR)
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("cid", ["e4", "e10"])
def test_every_stage_vs_fp64_oracle(T, cid, impl):
    """`forward_with_stages`: every recorded activation against the oracle's `stages` (1e-5 of the stage's maximum, the bar
    of tests/test_gpu_parity.py).  "force" is read from channels [0, 64) of the head's input: this pins which buffer the
    ping-pong of the force branch ends in (e4: three ResBlocks, e10: two, next to the copied pattern half)."""
    m, LR = _eval_model(T, cid, impl)
    y, stages = m.forward_with_stages(LR)
    ref, st64 = A.eval_ref(cid)
    st64 = dict(st64)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in A.case_data(cid)[1].items()}
    f = st64["force_in"]
    for i in range(A.case_cfg(cid)["forceFeatureExtraLayerCnt"] - 1):     # "res{i}": the ResBlocks in front of the last
        with torch.no_grad():
            f = st64[f"res{i}"] = O.resblock_forward(sd64, f"forceFeatureExtra_layer.{i}", f)
    assert set(stages) == set(st64), sorted(set(stages) ^ set(st64))
    worst = ("", 0.0)
    for name, t in stages.items():
        assert t.shape == st64[name].shape, name
        e = GC.relerr(t, st64[name])
        worst = max(worst, (name, e), key=lambda v: v[1])
        assert e < A.TOL, (name, e)
    print(f"[arch {cid} {impl} stages] {worst[1]:.1e} ({worst[0]}, worst of {len(stages)})")
    _check_image(f"{cid} {impl} with stages", y, cid)
    assert torch.equal(y, m(LR))


# ----------------------------------------------------------------------------------------------------------- train
TRAIN_RUNS = ([("fp16x3", c, b) for c, b in A.TRAIN_CASES]
              + [(impl, c, b) for impl in ("f32", "bf16x6") for c, b in A.TRAIN_CASES if c in ("t1", "t5")])


@pytest.mark.parametrize("impl,cid,b", TRAIN_RUNS)
def test_train_step_vs_fp64_oracle(T, impl, cid, b):
    """Loss, running statistics, ReLU pattern and every parameter gradient (1e-5) against the fp64 oracle on the device's
    pattern: the stem loop, the fuse conv's data gradient split over T stems, the ResBlock / MSRB loops both ways."""
    cfg = A.case_cfg(cid)
    _, worst = GC.train_step_vs_oracle(T, cfg, b, A.train_seed(cid, b), tol=1e-5, impl=impl, record=A.train_record(cid, b))
    print(f"[arch {cid} B={b} {impl} train] {worst[0]:.1e} ({worst[1]})")


@pytest.mark.parametrize("cid,b", [(c, b) for c, b in A.TRAIN_CASES if c in ("t1", "t3")])
def test_train_step_bf16_storage_vs_bf16_emulating_oracle(T, cid, b):
    GC.bf16_train_step_vs_emulating_oracle(T, A.case_cfg(cid), b, A.train_seed(cid, b))


@pytest.mark.parametrize("cid,b", [(c, b) for c, b in A.TRAIN_CASES if c in ("t1", "t3")])
def test_taxel_gradient_vs_fp64_oracle(T, cid, b):
    """LR.requires_grad_(): all 3T channels of LR.grad (frame t = channels 3t .. 3t+2, its stem's data gradient; frame 0
    also takes the force stem's) against the fp64 oracle's on the device's ReLU pattern, 1e-5 of the gradient's maximum
    (tests/test_gpu_scale_factors.py::test_taxel_gradient_vs_fp64_oracle)."""
    import test_gpu_input_grad as IG
    cfg, sd, LR, HR = A.case_data(cid, b)
    m, eng = IG._model(T, cfg, sd, "fp16x3")
    x = LR.cuda().requires_grad_(True)
    F.mse_loss(m(x), HR.cuda()).backward()
    assert x.grad is not None and x.grad.shape == x.shape == (b, 3 * cfg["seqsCnt"], 4, 4)
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    (g64,) = IG.oracle_input_grad(sd, LR, HR, A.SF, masks=masks)
    assert bool((g64.abs().amax(dim=(0, 2, 3)) > 0).all())             # every channel has a gradient to get wrong
    e = GC.relerr(x.grad, g64)
    print(f"[arch {cid} B={b} taxel grad] {e:.1e}")
    assert e < 1e-5, e


def test_graphed_train_step_t3_bit_identical_to_plain(T):
    """GraphedTrainStep on t3 (5 stems, 3 ResBlocks), B = 3: one eager warm-up step and three replays of ONE capture leave
    the loss dict of every step, the parameters, the Adam state and the buffers bit-identical to `train_one_iter`."""
    import test_gpu_train_graph as G
    from tactilesr_amd.train import tactileSR_train as TR
    from tactilesr_amd.train.graph import GraphedTrainStep
    cfg = A.case_cfg("t3")
    batches = G._batches(4, 3, cfg)
    ma, oa, sa, conf = G._setup("fp16x3", cfg)
    mg, og, sg, _ = G._setup("fp16x3", cfg)
    gstep = GraphedTrainStep(mg, og, conf, warmup=1)
    for i, b in enumerate(batches):
        da, dg = TR.train_one_iter(ma, oa, b, conf), gstep(b)
        assert set(da) == set(dg)
        for k in da:
            assert torch.equal(da[k], dg[k]), (i, k, float(da[k]), float(dg[k]))
        for s in (sa, sg):
            s.iter_update()
    assert gstep.captures == 1
    G._assert_same_state(ma, oa, mg, og)


# -------------------------------------------------------------------------------------------------------- refusals
def _assert_untouched(m, before):
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
@pytest.mark.parametrize("M,R", [(0, 1), (1, 0), (0, 0)])
def test_train_forward_without_a_block_is_refused_before_any_launch(T, M, R, impl):
    """The train step needs one MSRB and one ResBlock.  The refusal comes before the first launch: every parameter and
    buffer, running statistics and num_batches_tracked included, is bit-identical afterwards (it once came after the
    stems and the fuse conv had advanced their running statistics)."""
    from tactilesr_amd import _lib
    cfg = A.cfg_of(2, M, R)
    sd, LR, _ = GC.step_data(cfg, 3, 9500 + 2 * M + R)
    m = T.TactileSR(**cfg)
    m.train_impl = impl
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with pytest.raises(_lib.TactileSRHipError, match="train path needs (pattern|force)FeatureExtraLayerCnt >= 1"):
        m(LR.cuda())
    _assert_untouched(m, before)


@pytest.mark.parametrize("grid,axes", [((3, 5), 3), ((4, 2), 3), ((1, 4), 3), ((5, 5), 3), ((4, 4), 1), ((4, 4), 4)])
def test_other_grids_and_axis_counts_are_refused_before_any_launch(T, grid, axes):
    """Eval, train and `forward_with_stages` on a device tensor: a grid other than 4 x 4 (the reference's fixed (4sf, 4sf)
    output resize) and axisCnt != 3 (the 3-axis stem kernels) raise, and the state is untouched."""
    from tactilesr_amd import _lib
    m = T.TactileSR(axisCnt=axes, **A.cfg_of(2, 1, 1)).cuda()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.rand(3, 2 * axes, *grid).cuda()
    match = "axisCnt.*3-axis" if axes != 3 else "taxel grid .*resize"
    for mode in ("eval", "train", "stages"):
        m.train(mode == "train")
        with pytest.raises(_lib.TactileSRHipError, match=match):
            m.forward_with_stages(x) if mode == "stages" else m(x)
    _assert_untouched(m, before)
