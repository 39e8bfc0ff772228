"""Host-only checks of the single SR-loss path of the train step: ``SRLossSpec.from_config`` against the four config
parsers it is built from, and the rule of the report dict (``sr_loss_report``) on hand-made ``SRLossTerms`` for every
combination of {plain MSE / another criterion} x {SSIM off / on} x {degradation off / on} x {no weights / weights}."""
import dataclasses
import itertools

import pytest
import torch

import tactilesr_amd.functional as Fh
from tactilesr_amd._lib import TactileSRHipError as ERR
from tactilesr_amd.functional import SRLossTerms
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.tactileSR_train import SRLossSpec

BASE = TR.default_config()
NAN, INF = float("nan"), float("inf")
DEG = dict(degradation_loss_weight=0.1, degradation_gamma=0.7)
ALL_ON = dict(ssim_loss_weight=0.1, ssim_window=7, ssim_sigma=1.0, ssim_data_range=10.0, pixel_loss="huber",
              pixel_loss_param=0.5, contact_loss_weight=4.0, contact_threshold=0.5, degradation_channel=1,
              degradation_gain=2.0, sample_weight_norm="batch", **DEG)
TABLE = {
    "defaults": {},
    "ssim term": dict(ssim_loss_weight=0.1, ssim_window=7, ssim_sigma=1.0, ssim_data_range=10.0),
    "global ssim": dict(ssim_loss_weight=1, ssim_window=0),
    "pixel criterion": dict(pixel_loss="Huber", pixel_loss_param=0.5, contact_loss_weight=4, contact_threshold=0.5),
    "pixel parameter default": dict(pixel_loss="charbonnier"),
    "contact weight on the plain mse": dict(contact_loss_weight=2.0),
    "degradation term, channel and gain defaults": DEG,
    "degradation term, gamma from the batch": dict(degradation_loss_weight=2),
    "degradation channel and gain": dict(DEG, degradation_channel=0, degradation_gain=0.0),
    "degradation defaults follow axisCnt and HR_scale_num": dict(DEG, seqsCnt=7, axisCnt=3, HR_scale_num=4),
    "degradation keys unread when off": dict(degradation_gamma=-1, degradation_channel=99, degradation_gain=NAN),
    "batch norm": dict(sample_weight_norm="batch"),
    "everything": ALL_ON,
}


@pytest.mark.parametrize("name", list(TABLE))
def test_from_config_is_the_four_parsers_field_by_field(name):
    conf = dict(BASE, **TABLE[name])
    s = SRLossSpec.from_config(conf)
    assert (s.ssim_weight, s.window, s.sigma, s.data_range) == TR.ssim_loss_config(conf)
    assert (s.pixel_kind, s.pixel_param, s.fg_weight, s.fg_threshold) == TR.pixel_loss_config(conf)
    assert (s.deg_weight, s.deg_gamma, s.deg_channel, s.deg_gain) == TR.degradation_loss_config(conf)
    assert s.sample_weight_norm == TR.sample_weight_config(conf)
    assert s.plain_mse == TR.pixel_is_plain_mse(TR.pixel_loss_config(conf))
    names = {f.name for f in dataclasses.fields(s)}
    assert names >= {"ssim_weight", "window", "sigma", "data_range", "pixel_kind", "pixel_param", "fg_weight", "fg_threshold",
                     "deg_weight", "deg_gamma", "deg_channel", "deg_gain", "sample_weight_norm"}


def test_the_defaults_are_the_reference_loss():
    s = SRLossSpec.from_config(BASE)
    assert s.plain_mse and s.ssim_weight == 0 and s.deg_weight == 0 and s.deg_gain is None and s.sample_weight_norm == "sum"
    assert (s.window, s.sigma, s.data_range) == (11, 1.5, 1.0)
    on = SRLossSpec.from_config(dict(BASE, **DEG))
    assert (on.deg_channel, on.deg_gain) == (2, 10.0)               # the z axis of the first frame, HR_scale_num
    assert not SRLossSpec.from_config(dict(BASE, pixel_loss="l1")).plain_mse
    assert not SRLossSpec.from_config(dict(BASE, contact_loss_weight=1)).plain_mse


def test_equal_configs_give_equal_hashable_specs_and_every_key_counts():
    conf = dict(BASE, **ALL_ON)
    a, b = SRLossSpec.from_config(conf), SRLossSpec.from_config(dict(conf))
    assert a == b and hash(a) == hash(b) and {a: 1}[b] == 1 and a is not b
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.ssim_weight = 0.2
    changed = dict(ssim_loss_weight=0.2, ssim_window=9, ssim_sigma=1.5, ssim_data_range=1.0, pixel_loss="charbonnier",
                   pixel_loss_param=0.25, contact_loss_weight=1.0, contact_threshold=0.25, degradation_loss_weight=0.2,
                   degradation_gamma=0.9, degradation_channel=2, degradation_gain=0.0, sample_weight_norm="sum")
    assert set(changed) == set(ALL_ON)
    for k, v in changed.items():
        assert SRLossSpec.from_config(dict(conf, **{k: v})) != a, k
    assert SRLossSpec.from_config(dict(conf, lr=0.5, train_batch_size=2)) == a      # not a loss key


BAD = {
    TR.pixel_loss_config: [dict(pixel_loss="l3"), dict(pixel_loss=None), dict(pixel_loss="charbonnier", pixel_loss_param=0),
                           dict(pixel_loss="huber", pixel_loss_param=INF), dict(pixel_loss="huber", pixel_loss_param="x"),
                           dict(contact_loss_weight=-1), dict(contact_loss_weight=INF), dict(contact_loss_weight="x"),
                           dict(contact_threshold=NAN)],
    TR.degradation_loss_config: [dict(degradation_loss_weight=NAN), dict(degradation_loss_weight=INF),
                                 dict(degradation_loss_weight="x"), dict(DEG, degradation_gamma=0),
                                 dict(DEG, degradation_gamma=-0.7), dict(DEG, degradation_gamma=NAN),
                                 dict(DEG, degradation_gamma=INF), dict(DEG, degradation_gamma=2e6),
                                 dict(DEG, degradation_gamma="wide"), dict(DEG, degradation_gamma=torch.ones(4)),
                                 dict(DEG, degradation_channel=3), dict(DEG, degradation_channel=-1),
                                 dict(DEG, degradation_channel=1.0), dict(DEG, degradation_channel=True),
                                 dict(DEG, degradation_gain=NAN), dict(DEG, degradation_gain=INF),
                                 dict(DEG, degradation_gain="x")],
    TR.sample_weight_config: [dict(sample_weight_norm="mean"), dict(sample_weight_norm=None), dict(sample_weight_norm=1),
                              dict(sample_weight_norm="labeled")],
}


@pytest.mark.parametrize("parser", list(BAD), ids=[p.__name__ for p in BAD])
def test_what_a_parser_refuses_from_config_refuses(parser):
    for bad in BAD[parser]:
        conf = dict(BASE, **bad)
        with pytest.raises(ERR):
            parser(conf)
        with pytest.raises(ERR):
            SRLossSpec.from_config(conf)


# ------------------------------------------------------------------------------------------------------------ the report dict
B = 4
# the rule: total_loss always; the pixel term under mse_loss / pixel_loss unless the loss is the plain MSE alone; ssim,
# degradation_loss and labeled_weight with their terms.  Keys: (plain, ssim, degradation, weighted).
EXPECTED_KEYS = {
    (True, False, False, False): {"total_loss"},
    (True, False, False, True): {"total_loss", "mse_loss", "labeled_weight"},
    (True, False, True, False): {"total_loss", "mse_loss", "degradation_loss"},
    (True, False, True, True): {"total_loss", "mse_loss", "degradation_loss", "labeled_weight"},
    (True, True, False, False): {"total_loss", "mse_loss", "ssim"},
    (True, True, False, True): {"total_loss", "mse_loss", "ssim", "labeled_weight"},
    (True, True, True, False): {"total_loss", "mse_loss", "ssim", "degradation_loss"},
    (True, True, True, True): {"total_loss", "mse_loss", "ssim", "degradation_loss", "labeled_weight"},
    (False, False, False, False): {"total_loss", "pixel_loss"},
    (False, False, False, True): {"total_loss", "pixel_loss", "labeled_weight"},
    (False, False, True, False): {"total_loss", "pixel_loss", "degradation_loss"},
    (False, False, True, True): {"total_loss", "pixel_loss", "degradation_loss", "labeled_weight"},
    (False, True, False, False): {"total_loss", "pixel_loss", "ssim"},
    (False, True, False, True): {"total_loss", "pixel_loss", "ssim", "labeled_weight"},
    (False, True, True, False): {"total_loss", "pixel_loss", "ssim", "degradation_loss"},
    (False, True, True, True): {"total_loss", "pixel_loss", "ssim", "degradation_loss", "labeled_weight"},
}


@pytest.mark.parametrize("plain,ssim,deg,weighted", list(itertools.product((True, False), (False, True), (False, True),
                                                                           (False, True))))
def test_report_dict_rule(plain, ssim, deg, weighted, monkeypatch):
    conf = dict(BASE, **({} if plain else {"pixel_loss": "l1"}), **({"ssim_loss_weight": 0.1} if ssim else {}),
                **(DEG if deg else {}))
    spec = SRLossSpec.from_config(conf)
    g = torch.Generator().manual_seed(3)
    scale = torch.tensor([1.6, 0.0, 1.6, 0.8]) if weighted else None
    terms = SRLossTerms(loss=torch.tensor(1.25), dy=None, pixel=torch.tensor(0.75),
                        ssim=torch.rand(B, generator=g) if ssim else None, q=torch.rand(B, generator=g) if deg else None,
                        pix_b=torch.rand(B, generator=g) if weighted else None, scale=scale,
                        stats=torch.tensor([2.5, 3.0]) if weighted else None)
    means = []

    def mean(v, s=None):                                            # weighted_mean without the launch
        means.append((v, s))
        return ((v * s).sum() / v.shape[0]).reshape(1)
    monkeypatch.setattr(Fh, "weighted_mean", mean)
    d = TR.sr_loss_report(spec, terms)
    assert set(d) == EXPECTED_KEYS[plain, ssim, deg, weighted]
    assert d["total_loss"] is terms.loss
    alone = not (ssim or deg or weighted)
    if not (plain and alone):
        assert d["mse_loss" if plain else "pixel_loss"] is (terms.loss if alone else terms.pixel)
    if ssim and weighted:                                           # the one extra launch of the report
        assert len(means) == 1 and means[0][0] is terms.ssim and means[0][1] is scale
        assert float(d["ssim"]) == float((terms.ssim * scale).sum() / B) and d["ssim"].dim() == 0
    else:
        assert not means
        if ssim:
            assert torch.equal(d["ssim"], terms.ssim.mean())
    if deg:
        assert torch.equal(d["degradation_loss"], terms.q.mean())
    if weighted:
        assert float(d["labeled_weight"]) == 2.5 / B
