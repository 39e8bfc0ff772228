"""GPU check of the SR training loss over every combination of its terms: {plain MSE / another pixel criterion} x
{SSIM off / on} x {degradation off / on} x {no weights / per-sample weights}.  For each of the 16 the eager step
(``train_cal_loss`` / ``train_one_iter``) and the graph-captured one (``GraphedTrainStep``) must

  (a) issue exactly the loss launches documented in ``functional.sr_loss_fwd_bwd``'s docstring,
  (b) have the loss and every parameter gradient of ``sr_loss_fwd_bwd`` + the engine's backward driven by hand, bit for bit,
  (c) agree with each other bit for bit: the same report keys and values, parameters and Adam state, from one capture.

Only public entry points are used.  Smallest shapes: TactileSR(10, 1, 3, 1, 1), B = 4, 4x4 taxels, 100x100 HR, bf16."""
import itertools
import math

import pytest
import torch

import _sample_weight_cases as WC
import _ssim_cases as SC
import tactilesr_amd
import tactilesr_amd.functional as Fh
from tactilesr_amd import optim
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

pytestmark = pytest.mark.gpu

bits = WC.bits
LAM_S, LAM_D, GAMMA = 0.1, 0.1, 0.7
W4 = (1.0, 0.0, 1.0, 0.5)
COMBOS = list(itertools.product((True, False), (False, True), (False, True), (False, True)))      # plain, ssim, deg, weighted
IDS = ["-".join(("mse" if p else "l1", "ssim" if s else "nossim", "deg" if d else "nodeg", "w" if w else "now"))
       for p, s, d, w in COMBOS]


def _conf(plain, ssim, deg):
    c = TR.default_config()
    if not plain:
        c["pixel_loss"] = "l1"
    if ssim:
        c.update(ssim_loss_weight=LAM_S, ssim_data_range=10.0)
    if deg:
        c.update(degradation_loss_weight=LAM_D, degradation_gamma=GAMMA)
    return c


def _model(seed=42):
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR(10, 1, 3, 1, 1).cuda().train()
    m.train_impl = "bf16"
    return m


def _batch(weighted, seed=11, weights=W4):
    """Random taxels and a contact-like HR (blobs of amplitude <= 100 raw); with weights, the HR of a zero-weight sample is NaN."""
    g = torch.Generator().manual_seed(seed)
    LR, HR = torch.rand(4, 3, 4, 4, generator=g) * 8, SC.blobs(4, 100, 100, g) * 10
    if not weighted:
        return LR.cuda(), HR.cuda()
    w = torch.tensor(weights, dtype=torch.float32)
    HR[w == 0] = WC.NAN
    return LR.cuda(), HR.cuda(), None, w.cuda()


def _expected_launches(plain, ssim, deg, weighted):
    """The launch sequence of ``sr_loss_fwd_bwd``'s docstring, after the target preparation of ``_prep``; with weights and
    an SSIM term the step's report adds the weighted SSIM mean, a third ``tsr_weighted_mean``."""
    if weighted:
        return (["tsr_target_prep", "tsr_sample_scale", "tsr_pixel_loss_ps_fwd_bwd"] + (["tsr_ssim_fwd_bwd_ps"] if ssim else []) +
                (["tsr_degrade_fwd_bwd"] if deg else []) + ["tsr_weighted_mean"] * (3 if ssim else 1))
    return (["tsr_target_prep", "tsr_mse_fwd_bwd" if plain else "tsr_pixel_loss_fwd_bwd"] + (["tsr_ssim_fwd_bwd"] if ssim else []) +
            (["tsr_degrade_fwd_bwd"] if deg else []))


def _expected_keys(plain, ssim, deg, weighted):
    keys = {"total_loss"}
    if not plain or ssim or deg or weighted:
        keys.add("mse_loss" if plain else "pixel_loss")
    return keys | ({"ssim"} if ssim else set()) | ({"degradation_loss"} if deg else set()) | ({"labeled_weight"} if weighted else set())


@pytest.mark.parametrize("plain,ssim,deg,weighted", COMBOS, ids=IDS)
def test_eager_step_launches_and_bits(plain, ssim, deg, weighted, monkeypatch):
    conf, batch = _conf(plain, ssim, deg), _batch(weighted)
    names, real = [], Fh.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    m = _model()
    with monkeypatch.context() as mp:
        mp.setattr(Fh, "call", spy)
        loss, parts = TR.train_cal_loss(m, batch, conf)
    assert names == _expected_launches(plain, ssim, deg, weighted)                  # (a)
    assert set(parts) == _expected_keys(plain, ssim, deg, weighted) and parts["total_loss"] is loss
    if not plain and not (ssim or deg or weighted):
        assert parts["pixel_loss"] is loss
    m.zero_grad()
    loss.backward()
    r = _model()                                                                    # (b): the launches driven by hand on a twin
    LR, HR = TR._prep(batch, conf, "cuda")
    out = r(LR)
    lam_s, window, sigma, rng = TR.ssim_loss_config(conf)
    kind, param, fw, thr = TR.pixel_loss_config(conf)
    w_d, gamma, ch, gain = TR.degradation_loss_config(conf)
    l2, dy = Fh.sr_loss_fwd_bwd(out.detach().float(), HR, lam_s, rng, window, sigma, pixel_kind=kind, pixel_param=param,
                                fg_weight=fw, fg_threshold=thr, deg_weight=w_d, deg_z=LR[:, ch] if w_d else None,
                                deg_gamma=gamma, deg_gain=gain if w_d else 1.0,
                                sample_weight=batch[3] if weighted else None, sample_weight_norm=TR.sample_weight_config(conf))
    r.zero_grad()
    out.backward(dy.to(out.dtype))
    assert torch.equal(loss.detach(), l2[0]) and math.isfinite(float(loss.detach()))
    for (n, a), (_, b) in zip(m.named_parameters(), r.named_parameters()):
        assert torch.equal(bits(a.grad), bits(b.grad)), n
    assert max(float(p.grad.abs().max()) for p in m.parameters()) > 0


@pytest.mark.parametrize("plain,ssim,deg,weighted", COMBOS, ids=IDS)
def test_graphed_step_is_the_eager_step(plain, ssim, deg, weighted):
    conf = _conf(plain, ssim, deg)
    me, mg = _model(), _model()
    oe = optim.Adam(me.parameters(), lr=1e-3, weight_decay=1e-2)
    og = optim.Adam(mg.parameters(), lr=1e-3, weight_decay=1e-2)
    gstep = GraphedTrainStep(mg, og, dict(conf), warmup=1)
    for i, w in enumerate((W4, (0.0, 2.0, 0.25, 0.0), (1.0, 1.0, 1.0, 1.0))):       # one eager warm-up step, then two replays
        b = _batch(weighted, seed=20 + i, weights=w)
        pe = TR.train_one_iter(me, oe, b, conf)
        pg = gstep(b)
        assert set(pe) == set(pg) == _expected_keys(plain, ssim, deg, weighted), i
        for k in pe:
            assert torch.equal(pe[k].detach(), pg[k]) and math.isfinite(float(pg[k])), (i, k, float(pe[k].detach()), float(pg[k]))
    assert gstep.captures == 1
    for (n, a), (_, b) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = oe.state[a], og.state[b]
        assert float(sa["step"]) == float(sb["step"]) == 3, n
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    for (n, a), (_, b) in zip(me.named_buffers(), mg.named_buffers()):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("ssim", (False, True), ids=("nossim", "ssim"))
def test_a_zero_degradation_gain_means_zero_with_and_without_weights(ssim):
    """``degradation_gain = 0.0`` is passed to the launch as configured whatever the batch form: the pooled output is then 0
    and ``q_b`` the mean square of the z-taxels.  A 4-tuple of unit weights gives the 2-tuple step: the same degradation
    term and parameter gradients bit for bit (the per-sample pixel launch with unit scales has the unweighted launch's
    gradient), and the other report values to 1e-6 relative -- both are fp32 roundings of one sum, the weighted one rounded
    once from fp64 (``weighted_mean``), a few 6e-8 ulps apart."""
    conf = dict(_conf(False, ssim, True), degradation_gain=0.0)
    LR, HR = _batch(False)
    a, b = _model(), _model()
    la, pa = TR.train_cal_loss(a, (LR, HR), conf)
    lb, pb = TR.train_cal_loss(b, (LR, HR, None, torch.ones(4)), conf)
    la.backward()
    lb.backward()
    z2 = float((LR[:, 2].double() ** 2).mean())
    assert abs(float(pa["degradation_loss"]) - z2) <= 1e-6 * z2
    assert torch.equal(pa["degradation_loss"], pb["degradation_loss"])
    assert set(pb) == set(pa) | {"labeled_weight"} and float(pb["labeled_weight"]) == 1
    for k in pa:
        assert abs(float(pa[k]) - float(pb[k])) <= 1e-6 * abs(float(pa[k])), k
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(bits(p.grad), bits(q.grad)), n
