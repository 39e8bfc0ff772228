"""CPU checks of the degradation-consistency loss: the yardstick of tests/_degrade_cases.py against a brute-force sum over
the 16 explicit masks and against the reference's own outputs (tests/golden/degrade.npz), its closed-form gradient against
autograd, the fp32 restatement against the bar, the resize claim, the symbols and their refusals, the config keys, the
loader on device="cpu" and eval_func's default.  No GPU: refusals return before any device call."""
import inspect
import os
import re

import pytest
import torch

import _degrade_cases as DC
import tactilesr_amd.functional as Fh
from tactilesr_amd import _lib
from tactilesr_amd.data.device_loader import DeviceSRLoader
from tactilesr_amd.train import tactileSR_train as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = _lib.TactileSRHipError
CASES = [(H, W, B, s) for (H, W) in DC.SHAPES for B in DC.BATCHES for s in (False, True)]


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("gamma", DC.GAMMAS)
def test_restatement_is_the_sum_over_the_sixteen_masks(gamma):
    for signed in (False, True):
        y = DC.images(100, 100, 1, signed)
        D, _ = DC.restatement(y.double(), None, gamma)
        want = DC.brute_force(y[0, 0], gamma)
        assert float((D[0] - want).abs().max()) <= 1e-12 * float(want.abs().max()), (gamma, signed)


def test_restatement_is_the_reference_on_its_own_grid(golden):
    g = golden("degrade")
    y, gamma, want = torch.from_numpy(g["y"])[:, None], torch.from_numpy(g["gamma"]), torch.from_numpy(g["lr_deg_f32"]).double()
    assert y.shape == (6, 1, 100, 100) and sorted(set(gamma.tolist())) == [float(torch.tensor(v)) for v in DC.GAMMAS]
    assert (y[:4] >= 0).all() and (y[4:] < 0).any()
    D, _ = DC.restatement(y.double(), None, gamma.double())
    err = (D - want).abs().amax(dim=1) / want.abs().amax(dim=1)
    print(f"[degrade] restatement vs the reference's fp32 degradation_process: {float(err.max()):.2e} of the maximum")
    assert float(err.max()) <= 2e-6, err.tolist()


@pytest.mark.parametrize("H,W,B,signed", CASES)
def test_closed_form_is_autograd_and_fp32_stays_inside_its_bounds(H, W, B, signed):
    """fp32 throughout: below 1e-6 of the scale at gamma >= 0.7 (the 1e-5 bar keeps a factor of 10) and below 8e-6 at
    gamma = 0.05 (the coordinate's rounding in the exponent: tests/_degrade_cases.py); its sums alone, on rounded
    tables: below 1e-6 at every gamma."""
    worst, worst_sharp, worst_sums = DC.Worst(), DC.Worst(), DC.Worst()
    for gamma in DC.GAMMAS:
        for gain in DC.GAINS:
            ref = DC.reference(H, W, B, signed, gamma, gain)
            D, q, gy, gz = DC.autograd_grads(ref["y"], ref["z"], gamma, gain, torch.float64)
            for name, a, b in (("D", D, ref["D"]), ("q", q, ref["q"]), ("dy", gy, ref["dy"]), ("dz", gz, ref["dz"])):
                assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max()), (name, gamma, gain)
            fr = DC.fp32_fractions(ref)
            (worst if gamma >= DC.FP32_BAR_FROM else worst_sharp).take(fr)
            assert DC.fp32_bar(gamma) == (DC.FP32_BAR if gamma >= 0.7 else DC.FP32_SHARP_BAR) < DC.BAR
            assert max(fr.values()) <= DC.fp32_bar(gamma), (gamma, gain, fr)
            fs = DC.fp32_fractions(ref, tables="rounded")
            worst_sums.take(fs)
            assert max(fs.values()) <= DC.FP32_BAR, (gamma, gain, fs)
            assert bool(ref["q"].min() > 0) and not (not signed and bool((ref["y"] < 0).any()))
            assert not signed or B * H * W < 16 or bool((ref["y"] < 0).any())      # a few pixels may all be positive
    print(worst.line(f"fp32 throughout, gamma >= 0.7 (held to {DC.FP32_BAR:.0e}), {H}x{W} B={B}"))
    print(worst_sharp.line(f"fp32 throughout, gamma 0.05 (held to {DC.FP32_SHARP_BAR:.0e}), {H}x{W} B={B}"))
    print(worst_sums.line(f"fp32 sums on rounded tables, every gamma (held to {DC.FP32_BAR:.0e}), {H}x{W} B={B}"))


def test_per_sample_gammas_cover_the_range():
    g = DC.per_sample_gammas(67)
    assert g.dtype == torch.float32 and float(g.min()) < 0.1 and float(g.max()) > 20 and len(set(g.tolist())) == 67
    ref = DC.build_reference(DC.images(40, 40, 67, False), g, 10.0)
    assert max(DC.fp32_fractions(ref, tables="rounded").values()) <= DC.FP32_BAR
    assert max(DC.fp32_fractions(ref).values()) <= DC.fp32_bar(g) == DC.FP32_SHARP_BAR      # it holds sharp masks
    wide = g.clamp_min(1.0)                                         # the fp32 rounding of 0.7 is below 0.7
    ref = DC.build_reference(DC.images(40, 40, 67, False), wide, 10.0)
    assert max(DC.fp32_fractions(ref).values()) <= DC.fp32_bar(wide) == DC.FP32_BAR


@pytest.mark.parametrize("size", [40, 124])
def test_resized_blobs_carry_the_taxels_of_the_full_grid(size):
    """What lets the train step pool its resized target's grid: the operator on a bilinearly resized contact image is the
    operator on the 100x100 image, to 0.5 % of the largest taxel."""
    gen = torch.Generator().manual_seed(size)
    y = DC.blobs(8, 100, 100, gen).double()
    small = torch.nn.functional.interpolate(y, (size, size), mode="bilinear", align_corners=False)
    for gamma in DC.GAMMAS:
        D, _ = DC.restatement(y, None, gamma)
        d, _ = DC.restatement(small, None, gamma)
        err = float(((d - D).abs().amax(dim=1) / D.abs().amax(dim=1)).max())
        assert err <= 5e-3, (size, gamma, err)


def test_impulse_at_a_taxel_centre():
    y = torch.zeros(1, 1, 100, 100, dtype=torch.float64)
    y[0, 0, 37, 62] = 3.0
    for gamma in DC.GAMMAS:
        D, _ = DC.restatement(y, None, gamma, 10.0)
        assert abs(float(D[0, 4 * 1 + 2]) - 10.0 * 1e-4 * 3.0) <= 1e-15, gamma


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_entry_points_are_declared_at_abi_24():
    header = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    for name, n in (("tsr_degrade_fwd_bwd", 16), ("tsr_degrade_fwd_bwd_wgs", 17)):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
        assert decl, f"{name} is not declared in include/tactilesr_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n
        assert hasattr(_lib.load(), name)
    cap = re.search(r"^#define\s+TSR_DEGRADE_MAX_WGS\s+(\d+)", header, re.M)
    assert cap and int(cap.group(1)) == Fh.DEGRADE_MAX_WGS == DC.MAX_WGS
    top = re.search(r"^#define\s+TSR_DEGRADE_GAMMA_MAX\s+(\S+)", header, re.M)
    assert top and float(top.group(1)) == Fh.DEGRADE_GAMMA_MAX == DC.GAMMA_MAX
    assert Fh.DEGRADE_MAX_HW == DC.MAX_HW == 128
    assert os.path.exists(os.path.join(REPO, "tactilesr_amd", "csrc", "degrade_loss.hip"))
    assert _lib.ABI_VERSION == 24 and _lib.load().tsr_abi_version() == 24


def _fake_ptrs(a):
    addr = dict(y=1 << 20, z=2 << 20, gamma_dev=3 << 20, lr_deg=4 << 20, q=5 << 20, dy=6 << 20, dz=7 << 20)
    ptrs = {k: (addr[k] if a[k] else 0) for k in addr}
    if a["dy"] == "y":
        ptrs["dy"] = addr["y"]
    elif a["dy"] == "y+":
        ptrs["dy"] = addr["y"] + 4 * a["H"] * a["W"]
    return ptrs


@pytest.mark.parametrize("label,over", DC.REFUSALS, ids=[r[0] for r in DC.REFUSALS])
def test_refusals_need_no_device(label, over):
    """Status 1 before any device call: the pointers are fake addresses nothing may dereference."""
    a = dict(DC.BASE_ARGS, **over)
    assert DC.call_raw(_lib.load(), a, **_fake_ptrs(a)) == 1, label
    if "max_wgs" not in over:                                       # and the capped entry refuses the same
        assert DC.call_raw(_lib.load(), dict(a, max_wgs=4), **_fake_ptrs(a)) == 1, label


def test_refusal_table_covers_the_header():
    text = open(os.path.join(REPO, "include", "tactilesr_hip.h")).read()
    para = text[text.index("Degradation-consistency loss"):text.index("int tsr_degrade_fwd_bwd_wgs")]
    assert "Refusals" in para
    keys = {k for _, over in DC.REFUSALS for k in over}
    assert keys >= {"y", "B", "H", "W", "gamma_all", "gain", "q", "z", "lr_deg", "dy", "dz", "z_bstride", "accumulate",
                    "dy_scale", "max_wgs"}
    assert not {r[0] for r in DC.REFUSALS} & {r[0] for r in DC.ACCEPTED}


def test_cpu_tensors_and_bad_arguments_are_refused():
    y, z = torch.zeros(2, 1, 8, 8), torch.zeros(2, 16)
    for fn in (lambda: Fh.degrade(y, 0.7), lambda: Fh.degradation_fwd_bwd(y, z, 0.7), lambda: Fh.degradation_loss(y, z, 0.7),
               lambda: Fh.sr_loss_fwd_bwd(y, y, deg_weight=0.1, deg_z=z, deg_gamma=0.7),
               lambda: Fh.sr_loss(y, y, 0.0, deg_weight=0.1, deg_z=z, deg_gamma=0.7)):
        with pytest.raises(ERR):
            fn()
    assert Fh.degrade_gamma_arg(0.7, 4) == (None, 0.7) and Fh.degrade_gamma_arg(torch.tensor(2.0), 4) == (None, 2.0)
    g = torch.full((4,), 0.7)
    gd, ga = Fh.degrade_gamma_arg(g.double(), 4)
    assert gd.dtype == torch.float32 and torch.equal(gd, g) and ga == 0.0
    assert Fh.degrade_gamma_arg(1e6, 4) == (None, 1e6) and Fh.DEGRADE_GAMMA_MAX == DC.GAMMA_MAX == 1e6
    for bad in (0.0, -1.0, float("nan"), float("inf"), 2e6, "x", None, torch.ones(3), torch.ones(4, 1)):
        with pytest.raises(ERR):
            Fh.degrade_gamma_arg(bad, 4)
    sig = inspect.signature(Fh.sr_loss_fwd_bwd).parameters
    assert list(sig)[-4:] == ["deg_weight", "deg_z", "deg_gamma", "deg_gain"]
    assert [sig[k].default for k in list(sig)[-4:]] == [0.0, None, None, 1.0]
    assert list(inspect.signature(Fh.sr_loss).parameters)[-4:] == ["deg_weight", "deg_z", "deg_gamma", "deg_gain"]


# ------------------------------------------------------------------------------------------------------------ the train glue
def test_degradation_loss_config_keys():
    conf = TR.default_config()
    keys = {"degradation_loss_weight", "degradation_gamma", "degradation_channel", "degradation_gain"}
    assert not keys & set(conf)
    assert TR.degradation_loss_config(conf) == (0.0, None, None, None)
    assert TR.degradation_loss_config(dict(conf, degradation_loss_weight=0, degradation_gamma=-1,
                                           degradation_channel=99)) == (0.0, None, None, None)       # off: not read
    got = TR.degradation_loss_config(dict(conf, degradation_loss_weight=0.1, degradation_gamma=5))
    assert got == (0.1, 5.0, 2, 10.0) and [type(v) for v in got] == [float, float, int, float]
    assert TR.degradation_loss_config(dict(conf, degradation_loss_weight=2)) == (2.0, None, 2, 10.0)   # gamma from the batch
    seqs = dict(conf, seqsCnt=7, axisCnt=3, HR_scale_num=4, degradation_loss_weight=1, degradation_gamma=0.7)
    assert TR.degradation_loss_config(seqs) == (1.0, 0.7, 2, 4.0)
    assert TR.degradation_loss_config(dict(seqs, degradation_channel=20, degradation_gain=1)) == (1.0, 0.7, 20, 1.0)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(degradation_loss_weight=nan), dict(degradation_loss_weight=inf), dict(degradation_loss_weight="x"),
                dict(degradation_gamma=0), dict(degradation_gamma=-0.7), dict(degradation_gamma=nan),
                dict(degradation_gamma=inf), dict(degradation_gamma=2e6), dict(degradation_gamma="wide"), dict(degradation_gamma=torch.ones(4)),
                dict(degradation_channel=3), dict(degradation_channel=-1), dict(degradation_channel=1.0),
                dict(degradation_channel=True), dict(degradation_gain=nan), dict(degradation_gain=inf),
                dict(degradation_gain="x")):
        with pytest.raises(ERR):
            TR.degradation_loss_config({**conf, "degradation_loss_weight": 0.1, "degradation_gamma": 0.7, **bad})


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(2.0))

    def forward(self, x):
        return (self.w * x[:, :3].mean(dim=(1, 2, 3), keepdim=True)).expand(-1, 1, 40, 40).contiguous()


def test_a_bad_key_or_batch_raises_before_the_model_runs():
    ran = []

    class Spy(_Stub):
        def forward(self, x):
            ran.append(1)
            return super().forward(x)
    conf = TR.default_config()
    LR, HR = torch.rand(4, 3, 4, 4), torch.rand(4, 1, 100, 100)
    for c, batch in ((dict(conf, degradation_loss_weight=0.1), (LR, HR)),                         # no gamma anywhere
                     (dict(conf, degradation_loss_weight=0.1, degradation_gamma=-1), (LR, HR)),
                     (dict(conf, degradation_loss_weight=0.1, degradation_gamma=0.7, degradation_channel=5), (LR, HR)),
                     (dict(conf, degradation_loss_weight=0.1), (LR, HR, torch.ones(3))),           # gamma of another batch
                     (dict(conf, degradation_loss_weight=0.1), (LR, HR, torch.ones(4, 1))),
                     (dict(conf, degradation_loss_weight=0.1, degradation_gamma=0.7), (LR, HR, torch.ones(4), 1))):
        with pytest.raises(ERR):
            TR.train_cal_loss(Spy(), batch, c)
    assert not ran


def test_eval_func_default_is_unchanged_on_a_stub():
    sig = inspect.signature(TR.eval_func).parameters
    assert list(sig)[-1] == "degradation" and sig["degradation"].default is False
    conf = TR.default_config()
    g = torch.Generator().manual_seed(71)
    LR, HR = torch.rand(12, 3, 4, 4, generator=g) * 8, torch.rand(12, 1, 100, 100, generator=g) * 100
    gam = torch.rand(12, generator=g) + 0.5
    saved = Fh.mse_loss, Fh.psnr_ssim, Fh.prepare_target, Fh.degradation_fwd_bwd
    Fh.mse_loss = lambda y, t: ((y - t) ** 2).mean()
    Fh.psnr_ssim = lambda y, t, m, reference_quirk=True: (-(y - t).abs().mean((1, 2, 3)), (y * t).mean((1, 2, 3)))
    Fh.prepare_target = lambda h, s, f: h[:, :, 30:70, 30:70] / s
    calls = []

    def fake(y, z, gamma, gain=1.0, **kw):                          # the yardstick in place of the launch
        calls.append((z.clone(), gamma, gain))
        return (DC.restatement(y.double(), z.double(), gamma, gain)[1].float(),)
    Fh.degradation_fwd_bwd = fake
    try:
        base = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), conf)
        off = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), conf, degradation=False)
        three = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu", gamma=gam), conf)     # a 3-tuple, score off
        assert base == off == three and len(base) == 3 and not calls
        with pytest.raises(ERR):                                    # no gamma anywhere
            TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), conf, degradation=True)
        on = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu"), dict(conf, degradation_gamma=0.7),
                          degradation=True)
        assert on[:3] == base and len(on) == 4 and len(calls) == 3
        assert all(c[1] == 0.7 and c[2] == 10.0 for c in calls) and torch.equal(torch.cat([c[0] for c in calls]), LR[:, 2])
        out = _Stub()(LR).detach().double()
        want = sum(float(DC.restatement(out[i:i + 4], LR[i:i + 4, 2].double(), 0.7, 10.0)[1].mean()) for i in (0, 4, 8)) / 3
        assert abs(on[3] - want) <= 1e-6 * want
        calls.clear()
        per = TR.eval_func(_Stub(), DeviceSRLoader(LR, HR, 4, device="cpu", gamma=gam), dict(conf, degradation_gamma=0.7),
                           degradation=True)                        # the batch's gamma overrides the key
        assert torch.equal(torch.cat([c[1] for c in calls]), gam) and per[:3] == base and per[3] != on[3]
    finally:
        Fh.mse_loss, Fh.psnr_ssim, Fh.prepare_target, Fh.degradation_fwd_bwd = saved


# ------------------------------------------------------------------------------------------------------------------ the loader
def _set(n=11):
    g = torch.Generator().manual_seed(5)
    return torch.rand(n, 3, 4, 4, generator=g), torch.rand(n, 12, 12, generator=g), torch.arange(n, dtype=torch.float32) + 0.5


@pytest.mark.parametrize("kw", [dict(), dict(shuffle=True, seed=3), dict(shuffle=True, seed=3, drop_last=True),
                                dict(shuffle=True, seed=4, world_size=2, rank=1)], ids=["plain", "shuffle", "drop_last", "rank"])
def test_loader_without_gamma_is_the_loader_as_it_was(kw):
    LR, HR, gam = _set()
    a, b = DeviceSRLoader(LR, HR, 4, device="cpu", **kw), DeviceSRLoader(LR, HR, 4, device="cpu", gamma=gam, **kw)
    assert a.gamma is None
    for _ in range(2):                                              # two epochs: the generator state carries over
        n = 0
        for x, y in zip(a, b):
            assert len(x) == 2 and len(y) == 3 and a.last_index is None
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
            assert y[2].dtype == torch.float32 and torch.equal(y[2], b.gamma[b.last_index])
            assert torch.equal(y[0], b.LR[b.last_index])
            n += 1
        assert n == len(a) == len(b)
        assert torch.equal(a._gen.get_state(), b._gen.get_state())


@pytest.mark.parametrize("mode", ["random", "expand"])
def test_gamma_follows_the_index_under_augmentation(mode):
    LR, HR, gam = _set()
    kw = dict(shuffle=True, seed=9, augment="dihedral", augment_mode=mode)
    a, b = DeviceSRLoader(LR, HR, 4, device="cpu", **kw), DeviceSRLoader(LR, HR, 4, device="cpu", gamma=gam, **kw)
    seen = []
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(a.last_index, b.last_index)
        assert torch.equal(a.last_ops, b.last_ops) and torch.equal(y[2], gam[b.last_index])
        seen += b.last_index.tolist()
    assert torch.equal(a._gen.get_state(), b._gen.get_state())
    assert sorted(seen) == sorted(list(range(11)) * (8 if mode == "expand" else 1))


def test_loader_gamma_arguments():
    LR, HR, gam = _set()
    for bad in (gam[:5], gam.view(-1, 1)):
        with pytest.raises(ERR):
            DeviceSRLoader(LR, HR, 4, device="cpu", gamma=bad)
    ld = DeviceSRLoader(LR, HR, 4, device="cpu", gamma=gam.double().numpy())
    assert ld.gamma.dtype == torch.float32 and torch.equal(ld.gamma, gam)
    entries = [[{"LR": LR[i], "HR": HR[i], "alphaBeta": torch.tensor([1.0, 2.0, float(gam[i])])}] for i in range(11)]
    assert DeviceSRLoader.from_entries(entries, 4, device="cpu").gamma is None
    ld = DeviceSRLoader.from_entries(entries, 4, device="cpu", with_gamma=True)
    assert torch.equal(ld.gamma, gam) and len(next(iter(ld))) == 3
    sig = inspect.signature(DeviceSRLoader.from_file).parameters
    assert sig["with_gamma"].default is False
