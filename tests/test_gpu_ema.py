"""Weight EMA / SWA on the device: tsr_ema_multi / tsr_ema_multi_dev against the fp64 restatement under the derived
bound of tests/_ema_cases.py (raw-word operations bit for bit), then WeightEMA in the train step, the captured step,
applied(), eval_func, the checkpoint and recalibrate_bn.  Every kernel launch goes into NaN-prefilled buffers between
NaN guard bands and runs twice from the same bits (the harness of _ema_cases)."""
import ctypes

import pytest
import torch

import _ema_cases as EC
import _ssim_cases as SC
import tactilesr_amd
from tactilesr_amd import _lib, optim
from tactilesr_amd.ema import WeightEMA, recalibrate_bn
from tactilesr_amd.model.tactileSR_model import hold_bn_statistics
from tactilesr_amd.train import checkpoint as CK
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep

pytestmark = pytest.mark.gpu
U, ST, LD, SW = EC.UPDATE, EC.STORE, EC.LOAD, EC.SWAP
f32 = EC.as_f32


def _rand(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def _eq(a, b):
    return len(a) == len(b) and all(torch.equal(EC.bits(x), EC.bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("omd", EC.OMDS)
def test_sizes(omd):
    avg = [_rand(n, 100 + i) for i, n in enumerate(EC.SIZES)]
    src = [_rand(n, 200 + i) for i, n in enumerate(EC.SIZES)]
    got, after = EC.launch(avg, src, [0] * len(avg), U, omd)
    assert _eq(after, src)                                   # UPDATE only reads src
    worst = max(EC.check(f32(g), a, s, omd, label=f"n={a.numel()}") for g, a, s in zip(got, avg, src))
    print(f"[ema] sizes, omd {omd}: worst {worst:.3f} of the bound")
    if omd == 0.0:
        assert _eq(got, avg)
    dev, _ = EC.launch(avg, src, [0] * len(avg), U, omd, dev_form=True)
    assert _eq(dev, got)                                     # the device-scalar form: the same bits for the same float


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("which", ["avg", "src", "both"])
def test_alignment(which, off):
    sizes = (1, 3, 5, 257, 4097)
    avg = [_rand(n, 300 + i) for i, n in enumerate(sizes)]
    src = [_rand(n, 400 + i) for i, n in enumerate(sizes)]
    offs = dict(avg_off=off if which != "src" else 0, src_off=off if which != "avg" else 0)
    got, after = EC.launch(avg, src, [0] * len(avg), U, 0.25, **offs)
    assert _eq(after, src)
    for g, a, s in zip(got, avg, src):
        EC.check(f32(g), a, s, 0.25, label=f"{which}+{off} n={a.numel()}")
    aligned, _ = EC.launch(avg, src, [0] * len(avg), U, 0.25)
    assert _eq(got, aligned)                                 # the scalar path rounds like the 16-byte one
    a2, s2 = EC.launch(avg, src, [0] * len(avg), SW, 0.0, **offs)
    assert _eq(a2, src) and _eq(s2, avg)


def test_2100_distinct_records():
    base_a, base_s = _rand(4, 1), _rand(4, 2)
    avg = [base_a * (1 + i / 64) for i in range(2100)]
    src = [base_s * (1 + i / 32) for i in range(2100)]
    got, after = EC.launch(avg, src, [0] * 2100, U, 0.5)
    assert _eq(after, src)
    EC.check(torch.cat([f32(g) for g in got]), torch.cat(avg), torch.cat(src), 0.5, label="2100 records")


def _mixed():
    g = torch.Generator().manual_seed(5)
    ints = torch.randint(-2 ** 62, 2 ** 62, (700,), generator=g, dtype=torch.int64)
    ints[0], ints[1] = 7, -1
    src = [_rand(5000, 10), _rand(4100, 11), ints, _rand(9, 12)]
    avg = [_rand(5000, 20), _rand(4100, 21), torch.randint(-2 ** 62, 2 ** 62, (700,), generator=g, dtype=torch.int64),
           _rand(9, 22)]
    return avg, src, [0, 1, 1, 0]


def test_update_mixes_modes_in_one_launch():
    avg, src, modes = _mixed()
    got, after = EC.launch(avg, src, modes, U, 1e-3)
    assert _eq(after, src)
    for i in (0, 3):
        EC.check(f32(got[i]), avg[i], src[i], 1e-3, label=f"mode 0 tensor {i}")
        assert not torch.equal(got[i], EC.bits(src[i]))
    for i in (1, 2):
        assert torch.equal(got[i], EC.bits(src[i])), i       # mode 1: raw words, int64 as two words per element
    assert torch.equal(got[2].view(torch.int64), src[2])


def test_store_load_swap_move_raw_words():
    avg, src, modes = _mixed()
    got, after = EC.launch([None] * 4, src, modes, ST, 0.5)              # into the NaN prefill
    assert _eq(got, src) and _eq(after, src)
    got, after = EC.launch(avg, src, modes, LD, 0.5)
    assert _eq(got, avg) and _eq(after, avg)
    got, after = EC.launch(avg, src, modes, SW, 0.5)
    assert _eq(got, src) and _eq(after, avg)
    got, after = EC.launch(avg, src, modes, SW, 0.5, repeat=2)           # two SWAPs: the identity on bits
    assert _eq(got, avg) and _eq(after, src)
    got, after = EC.launch(avg, src, modes, SW, 0.5, dev_form=True)      # op selects, the scalar is not used
    assert _eq(got, src) and _eq(after, avg)


@pytest.mark.parametrize("omd", EC.OMDS)
def test_exact_cases(omd):
    a = [_rand(n, 30 + n) for n in (7, 4096, 4099)]
    a[0][3] = 0.0
    got, _ = EC.launch(a, [t.clone() for t in a], [0] * 3, U, omd)
    assert _eq(got, a)                                       # src == avg: unchanged bit for bit
    if omd == 1.0:
        got, _ = EC.launch([torch.zeros_like(t) for t in a], a, [0] * 3, U, omd)
        assert _eq(got, a)                                   # avg == 0, omd == 1: src exactly


@pytest.mark.parametrize("n", [64, 4100])
def test_non_finite_values_stay_in_their_element(n):
    avg, src = _rand(n, 1), _rand(n, 2)
    src[3], src[7], src[11] = float("nan"), float("inf"), -0.0
    avg[20], avg[24], avg[28] = float("nan"), -float("inf"), -0.0
    got, after = EC.launch([avg], [src], [0], U, 0.5)
    r = f32(got[0])
    EC.check(r, avg, src, 0.5, label="non-finite")           # NaN and Inf patterns equal the restatement's
    assert (~torch.isfinite(r)).nonzero().flatten().tolist() == [3, 7, 20, 24]
    assert torch.isnan(r[3]) and r[7] == float("inf") and torch.isnan(r[20]) and torch.isnan(r[24])     # Inf - Inf
    assert float(r[11]) == 0.5 * float(avg[11]) and float(r[28]) == 0.5 * float(src[28])
    assert _eq(after, [src])


@pytest.mark.parametrize("op", [U, SW])
def test_bad_records_are_skipped(op):
    avg = [_rand(8, 50 + i) for i in range(6)]
    src = [_rand(8, 60 + i) for i in range(6)]
    bad = {1: (0, 0), 2: (4097, 0), 3: (8, 2), 4: (8, -1)}
    got, after = EC.launch(avg, src, [0] * 6, op, 0.5, override=bad)
    for i in bad:
        assert torch.equal(got[i], EC.bits(avg[i])) and torch.equal(after[i], EC.bits(src[i])), i
    for i in (0, 5):                                          # the neighbours run as usual
        if op == U:
            EC.check(f32(got[i]), avg[i], src[i], 0.5)
            assert torch.equal(after[i], EC.bits(src[i])) and not torch.equal(got[i], EC.bits(avg[i]))
        else:
            assert torch.equal(got[i], EC.bits(src[i])) and torch.equal(after[i], EC.bits(avg[i]))


def test_refusals_leave_the_shadow_untouched():
    src = [_rand(9, 1), _rand(4100, 2)]
    g = EC.Guarded([None, None], src, [0, 0])
    lib = _lib.load()
    scalar = torch.tensor([0.5], dtype=torch.float32).cuda()
    I, F, null, t, s = ctypes.c_int, ctypes.c_float, ctypes.c_void_p(0), _lib.ptr(g.table), _lib.stream()
    for a in [(null, I(g.n_chunks), I(1)), (t, I(0), I(1)), (t, I(-1), I(1)), (t, I(g.n_chunks), I(-1)),
              (t, I(g.n_chunks), I(4))]:
        assert lib.tsr_ema_multi(*a, F(0.5), s) == 1 and lib.tsr_ema_multi_dev(*a, _lib.ptr(scalar), s) == 1
    for omd in (float("nan"), -1e-6, 1.0 + 2.0 ** -20, float("inf")):
        assert lib.tsr_ema_multi(t, I(g.n_chunks), I(1), F(omd), s) == 1
    assert lib.tsr_ema_multi_dev(t, I(g.n_chunks), I(1), null, s) == 1
    torch.cuda.synchronize()
    avg, after = g.read()
    assert all(bool((a == EC.SENTINEL).all()) for a in avg) and _eq(after, src)
    assert lib.tsr_ema_multi(t, I(g.n_chunks), I(1), F(0.5), s) == 0          # and the same table is accepted
    torch.cuda.synchronize()
    assert _eq(g.read()[0], src)


# ------------------------------------------------------------------------------------------ train step
CONF = TR.default_config()


def _model(seed=42):
    torch.manual_seed(seed)
    return tactilesr_amd.TactileSR(10, 1, 3, 1, 1).cuda().train()


def _batch(B=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (SC.blobs(B, 100, 100, g) * 10).cuda()


def _opt(m, lr=1e-3):
    return optim.Adam(m.parameters(), lr=lr, weight_decay=1e-2)


def _snap(m, opt=None):
    out = {k: EC.bits(v) for k, v in m.state_dict().items()}
    if opt is not None:
        for i, p in enumerate(m.parameters()):
            st = opt.state[p]
            out.update({f"adam.{i}.m": EC.bits(st["exp_avg"]), f"adam.{i}.v": EC.bits(st["exp_avg_sq"]),
                        f"adam.{i}.step": EC.bits(st["step"].float())})
    return out


def _shadow(e):
    return {k: EC.bits(v) for k, v in e.shadow.items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("path,buffers", [("fused", "copy"), ("fallback", "ema")])
def test_three_steps_follow_the_restatement_and_do_not_perturb_training(monkeypatch, path, buffers):
    if path == "fallback":
        monkeypatch.setattr(TR, "fused_clip_applies", lambda model, optimizer: False)
    m, r = _model(), _model()
    om, orr = _opt(m), _opt(r)
    e = WeightEMA(m, decay=0.999, warmup=10, buffers=buffers)
    assert e.launches == 1 and _same(_shadow(e), _snap(m)) and e._flat.data_ptr() % 16 == 0
    params = {n for n, _ in m.named_parameters()}
    for t in range(3):
        prev = {k: v.detach().cpu().clone() for k, v in e.shadow.items()}
        batch = _batch(seed=11 + t)
        TR.train_one_iter(m, om, batch, CONF, clip_grad_norm=1.0, ema=e)
        TR.train_one_iter(r, orr, batch, CONF, clip_grad_norm=1.0)
        assert e.updates == t + 1 and e.launches == t + 2 and e.table_builds == 1
        worst = 0.0
        for k, v in m.state_dict().items():
            v = v.detach().cpu()
            if v.dtype == torch.float32 and (k in params or buffers == "ema"):
                worst = max(worst, EC.check(e.shadow[k].cpu().reshape(-1), prev[k].reshape(-1), v.reshape(-1),
                                            1.0 - e.decay_at(t), label=f"step {t} {k}"))
            else:
                assert torch.equal(EC.bits(e.shadow[k]), EC.bits(v)), (t, k)
        print(f"[ema] {path} / buffers={buffers}, step {t}: worst {worst:.3f} of the bound")
        assert _same(_snap(m, om), _snap(r, orr)), f"step {t}: the average perturbed training"
    assert not _same(_shadow(e), _snap(m))
    assert all(int(e.shadow[k]) == 3 for k in e.shadow if k.endswith("num_batches_tracked"))


def test_graphed_step_matches_eager_bit_for_bit_with_a_warming_decay():
    batches = [_batch(seed=20 + t) for t in range(6)]
    m1, m2, m3 = _model(), _model(), _model()
    o1, o2, o3 = _opt(m1), _opt(m2), _opt(m3)
    e1 = WeightEMA(m1, decay=0.999, warmup=10)
    e2 = WeightEMA(m2, decay=0.999, warmup=10)
    g2 = GraphedTrainStep(m2, o2, CONF, warmup=1, ema=e2)
    g3 = GraphedTrainStep(m3, o3, CONF, warmup=1)                        # ema=None: the step as it was
    for t in range(4):                                                   # one eager warm-up call + three replays
        TR.train_one_iter(m1, o1, batches[t], CONF, ema=e1)
        g2(batches[t])
        g3(batches[t])
        # a decay frozen at the capture (update 1: 2/11) would part the shadows at t = 2
        assert _same(_shadow(e2), _shadow(e1)), f"step {t}: shadow"
        assert _same(_snap(m2, o2), _snap(m1, o1)), f"step {t}: parameters / optimizer state"
    assert g2.captures == 1 and g3.captures == 1
    assert (e2.updates, e2.launches, e2.table_builds) == (4, 5, 1) == (e1.updates, e1.launches, e1.table_builds)
    assert _same(_snap(m3, o3), _snap(m1, o1))
    assert o2.launches == o3.launches == o1.launches == 4               # the Adam launch count is today's
    assert g3._ema_omd is None and g3._ema_table is None and g2._ema_omd is not None
    # inside applied() a call is refused before any host state moves
    with e2.applied():
        with pytest.raises(_lib.TactileSRHipError, match="applied"):
            g2(batches[4])
    assert e2.updates == 4 and o2.launches == 4
    # another WeightEMA object recaptures: one eager call, then the capture
    e2b = WeightEMA(m2, decay=0.999, warmup=10)
    e1.reset()
    g2.ema = e2b
    for t in (4, 5):
        TR.train_one_iter(m1, o1, batches[t], CONF, ema=e1)
        g2(batches[t])
    assert g2.captures == 2 and e2b.updates == 2
    assert _same(_shadow(e2b), _shadow(e1)) and _same(_snap(m2, o2), _snap(m1, o1))


def _trained(steps=2, buffers="copy"):
    m = _model()
    o = _opt(m, lr=1e-5)      # small steps: two Adam steps at 1e-3 push this tiny network's eval output to all zero
    e = WeightEMA(m, decay=0.5, buffers=buffers)
    for t in range(steps):
        TR.train_one_iter(m, o, _batch(seed=30 + t), CONF, ema=e)
    return m, o, e


def test_applied_runs_the_model_on_the_average_and_restores_it():
    m, _, e = _trained()
    x = _batch(seed=40)[0]
    m.eval()
    with torch.no_grad():
        before = m(x).clone()                                # fills the eval plan with the weights' packs
    assert float(before.abs().max()) > 0                     # a dead output could not tell the weights from the average
    weights, shadow = _snap(m), _shadow(e)
    ptrs = [t.data_ptr() for t in m.state_dict().values()]
    fresh = _model(seed=7).eval()
    fresh.load_state_dict(e.shadow)
    with torch.no_grad():
        want = fresh(x)
        with e.applied():
            assert _same(_snap(m), shadow) and _same(_shadow(e), weights)
            inside = m(x).clone()
        after = m(x)
    assert torch.equal(inside, want)                         # a stale weight pack or plan would give `before`
    assert not torch.equal(inside, before)
    assert torch.equal(after, before) and _same(_snap(m), weights) and _same(_shadow(e), shadow)
    assert [t.data_ptr() for t in m.state_dict().values()] == ptrs
    # eval_func
    loader = [_batch(seed=50), _batch(seed=51)]
    plain = TR.eval_func(m, loader, CONF)
    assert TR.eval_func(m, loader, CONF, ema=None) == plain
    assert TR.eval_func(m, loader, CONF, ema=e) == TR.eval_func(fresh, loader, CONF) != plain
    assert _same(_snap(m), weights) and TR.eval_func(m, loader, CONF) == plain


def test_checkpoint_round_trip_on_the_device(tmp_path):
    m, o, e = _trained(buffers="ema")
    path = str(tmp_path / "ema.pth")
    CK.save_checkpoint(path, m, o, iteration=2, ema=e)
    m2 = _model(seed=9)
    e2 = WeightEMA(m2, decay=0.9)
    ck = CK.load_checkpoint(path, m2, _opt(m2), ema=e2)
    assert "ema_missing" not in ck and (e2.decay, e2.buffers, e2.updates) == (0.5, "ema", 2)
    assert all(v.is_cuda for v in e2.shadow.values()) and _same(_shadow(e2), _shadow(e)) and _same(_snap(m2), _snap(m))
    # the restored average goes on exactly like the original
    batch = _batch(seed=60)
    TR.train_one_iter(m, o, batch, CONF, ema=e)
    o2 = _opt(m2)
    CK.load_checkpoint(path, m2, o2, ema=e2)
    TR.train_one_iter(m2, o2, batch, CONF, ema=e2)
    assert _same(_shadow(e2), _shadow(e))


def test_recalibrate_bn_over_three_batches():
    m, c = _model(), _model()
    for net in (m, c):
        hold_bn_statistics(net.patternFeatureExtra_layer)      # the MSRB: 4 of the 7 BatchNorm layers
    bns = lambda net: [(n, b) for n, b in net.named_modules() if isinstance(b, torch.nn.BatchNorm2d)]
    held = {n for n, b in bns(m) if not b.training}
    assert held and len(held) < len(bns(m))
    loader = [_batch(seed=70 + k) for k in range(3)]
    # the per-batch statistics: three separate forwards with momentum 1.0 on a copy of the model
    for _, b in bns(c):
        b.momentum = 1.0
    stats = []
    with torch.no_grad():
        for LR, _ in loader:
            c(LR)
            stats.append({n: (b.running_mean.double().cpu(), b.running_var.double().cpu()) for n, b in bns(c)})
    before = _snap(m)
    m.eval()
    assert recalibrate_bn(m, loader, CONF) == 3
    assert not m.training and all(b.momentum == 0.1 and not b.training for _, b in bns(m))       # restored
    after = _snap(m)
    for n, b in bns(m):
        if n in held:
            assert all(torch.equal(after[f"{n}.{k}"], before[f"{n}.{k}"])
                       for k in ("running_mean", "running_var", "num_batches_tracked")), n
            continue
        assert int(b.num_batches_tracked) == 3
        for i, got in enumerate((b.running_mean, b.running_var)):
            want = sum(s[n][i] for s in stats) / 3
            err = float((got.double().cpu() - want).abs().max())
            assert err <= 1e-6 * float(want.abs().max()), (n, i, err, float(want.abs().max()))
    assert all(torch.equal(after[k], before[k]) for k, _ in m.named_parameters())
