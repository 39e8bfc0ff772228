"""CPU preconditions of tests/test_gpu_architectures.py (case tables: tests/_arch_cases.py): every case loads into the model,
has a finite, live fp64 output whose images are of one magnitude, trains on a ReLU pattern that is neither dead nor saturated,
and the dominance cases dominate.  These are CONDITIONS on the cases, never measurements of the code under test: a seed that
misses one is replaced, no bound is lowered.  Also here, without a device: the model-level refusals (taxel grid, axisCnt) come
before the device check and before any launch, and a refused train forward launches nothing."""
import pytest
import torch

import tactilesr_amd
from tactilesr_amd import _lib
import _arch_cases as A
from _infer_f16s import image_ratio

ALL_STEPS = [(c, A.B) for c in A.EVAL_IDS] + A.TRAIN_CASES


@pytest.mark.parametrize("cid,b", ALL_STEPS)
def test_state_dict_loads_strict(cid, b):
    cfg, sd, LR, HR = A.case_data(cid, b)
    m = tactilesr_amd.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    T, M, R = cfg["seqsCnt"], cfg["patternFeatureExtraLayerCnt"], cfg["forceFeatureExtraLayerCnt"]
    assert (len(m.inputLayer_pattern_list), len(m.patternFeatureExtra_layer), len(m.forceFeatureExtra_layer)) == (T, M, R)
    assert m.inputContact_layer[0].weight.shape == (64, 64 * T, 3, 3)
    assert LR.shape == (b, 3 * T, 4, 4) and HR.shape == (b, 1, 4 * A.SF, 4 * A.SF)


def test_tables_are_the_ones_the_gpu_tests_mean():
    assert A.FULL == ["e1", "e2", "e3", "e4", "e5", "e6"] and A.COPY == ["e7", "e8", "e9", "e10", "d1", "d2", "d3"]
    assert [A.EVAL[c][0] * 64 for c in A.FULL] == [192, 256, 320, 384, 576, 640]
    assert all(min(v[1:]) >= 1 for v in A.TRAIN.values())
    assert len(A.TRAIN_CASES) == 7 and len(set(A.SEED.values())) == len(A.SEED)
    for cid, (base, factors, _) in A.DOMINANCE.items():       # a dominance case is its base case but for the scaled tensors
        sd, sb = A.case_data(cid)[1], A.case_data(base)[1]
        assert set(factors) <= set(sd)
        for k in sd:
            assert torch.equal(sd[k], sb[k] * factors.get(k, 1.0) if k in factors else sb[k]), k
        assert torch.equal(A.case_data(cid)[2], A.case_data(base)[2])


@pytest.mark.parametrize("cid", A.EVAL_IDS)
def test_eval_reference_is_finite_live_and_of_one_magnitude(cid):
    ref, stages = A.eval_ref(cid)
    assert ref.shape == (A.B, 1, 4 * A.SF, 4 * A.SF) and bool(torch.isfinite(ref).all())
    assert all(bool(torch.isfinite(t).all()) for t in stages.values())
    assert float(ref.amax(dim=(1, 2, 3)).min()) > 0               # a dead-ReLU image would make the GPU test empty
    assert image_ratio(ref) < 4, image_ratio(ref)
    e = A.e_ref(cid)
    print(f"[arch {cid}] e_ref (torch fp32 CPU vs fp64) {e:.2e}, bar {A.eval_bar(cid):.2e}, image max ratio {image_ratio(ref):.2f}")
    if cid not in A.WIDE:     # conditioning: the flat bar is the one max(TOL, 4 * e_ref) gives (else: another seed)
        assert 4 * e <= A.TOL, e
    assert A.eval_bar(cid) ==(max(A.TOL, 4 * e) if cid in A.WIDE else A.TOL)


@pytest.mark.parametrize("cid", list(A.DOMINANCE))
def test_dominance_cases_dominate(cid):
    num, den, bound = A.DOMINANCE[cid][2]
    _, stages = A.eval_ref(cid)
    v = A.stage_max(stages, num) / (A.stage_max(stages, den) if den is not None else 1.0)
    print(f"[arch {cid}] max|{num}|" + (f" / max|{den}|" if den else "") + f" = {v:.4g} (condition: > {bound:g})")
    if den is None:
        assert v > bound
    else:
        assert v >= bound


@pytest.mark.parametrize("cid,b", ALL_STEPS)
def test_train_step_pattern_is_neither_dead_nor_saturated(cid, b):
    """Every ReLU stage of the oracle's train step has between 1 % and 99 % active elements."""
    loss, grads, ns, pre = A.train_record(cid, b)
    assert loss > 0 and pre
    frac = {k: float((p > 0).double().mean()) for k, p in pre.items()}
    lo, hi = min(frac, key=frac.get), max(frac, key=frac.get)
    print(f"[arch {cid} B={b}] active share {frac[lo]:.3f} ({lo}) .. {frac[hi]:.3f} ({hi})")
    assert 0.01 <= frac[lo] and frac[hi] <= 0.99, (lo, frac[lo], hi, frac[hi])
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


# ------------------------------------------------------------------------------------------------------------ refusals
def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _assert_untouched(m, before):
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in m.parameters())


def _calls(m, x):
    """The three model-level entry points, as (name, thunk)."""
    def ev():
        m.eval()
        return m(x)

    def tr():
        m.train()
        return m(x)

    def st():
        m.eval()
        return m.forward_with_stages(x)
    return [("eval", ev), ("train", tr), ("stages", st)]


@pytest.mark.parametrize("grid", [(3, 5), (4, 2), (1, 4), (5, 5)])
def test_other_taxel_grids_are_refused_before_the_device_check(grid):
    """The reference resizes its output to (4sf, 4sf) whatever the grid; this engine has no such resize.  A CPU tensor
    reaches the refusal: it comes before the "ROCm device" check, hence before any launch."""
    m = tactilesr_amd.TactileSR(**A.cfg_of(2, 1, 1))
    before = _state(m)
    x = torch.rand(2, 6, *grid)
    for name, fn in _calls(m, x):
        with pytest.raises(_lib.TactileSRHipError, match=r"taxel grid .*resize"):
            fn()
    _assert_untouched(m, before)
    m.eval()
    with pytest.raises(_lib.TactileSRHipError, match="no CPU fallback"):         # 4 x 4 goes on to the device check
        m(torch.rand(2, 6, 4, 4))


@pytest.mark.parametrize("axes", [1, 4])
def test_other_axis_counts_are_refused_before_the_device_check(axes):
    m = tactilesr_amd.TactileSR(axisCnt=axes, **A.cfg_of(2, 1, 1))
    before = _state(m)
    x = torch.rand(2, 2 * axes, 4, 4)
    for name, fn in _calls(m, x):
        with pytest.raises(_lib.TactileSRHipError, match="axisCnt.*3-axis"):
            fn()
    _assert_untouched(m, before)


@pytest.mark.parametrize("impl", ["fp16x3", "bf16"])
@pytest.mark.parametrize("M,R", [(0, 1), (1, 0), (0, 0)])
def test_refused_train_forward_launches_nothing(M, R, impl):
    """The train engine's "needs ... >= 1" refusals come before the first launch (dry run: the launch functions count)."""
    from test_bn_modes_cpu import _DryRun
    m = tactilesr_amd.TactileSR(**A.cfg_of(2, M, R)).train()
    m.train_impl = impl
    before = _state(m)
    eng = m.train_engine()
    with _DryRun() as dry, torch.no_grad():
        with pytest.raises(_lib.TactileSRHipError, match="train path needs (pattern|force)FeatureExtraLayerCnt >= 1"):
            eng.forward(torch.rand(3, 6, 4, 4))
        assert dry.trace == [], [t[0] for t in dry.trace]
    _assert_untouched(m, before)
    # the grid refusal holds on this entry point too (GraphedTrainStep calls it directly)
    with _DryRun() as dry, torch.no_grad():
        with pytest.raises(_lib.TactileSRHipError, match="taxel grid"):
            eng.forward(torch.rand(3, 6, 3, 5))
        assert dry.trace == []
