"""GPU checks of the graph-captured train step (tactilesr_amd.train.graph.GraphedTrainStep): the replayed step has the
plain ``train_one_iter``'s results bit for bit under an lr schedule that changes lr from step to step (loss, parameters,
Adam state, BatchNorm buffers), eval after graphed training sees the new weights, checkpoints written from graphed
training resume exactly, changed baked constants recapture, and the refusals hold."""
import time

import pytest
import torch

import tactilesr_amd
from tactilesr_amd import _lib, ddp, optim
from tactilesr_amd.train import tactileSR_train as TR
from tactilesr_amd.train.graph import GraphedTrainStep
from tactilesr_amd.train.lr_scheduler import LRWarmupScheduler

pytestmark = pytest.mark.gpu

SEQS = dict(scale_factor=25, seqsCnt=8)


def _setup(impl="fp16x3", cfg=None, seed=42, sched=True):
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR(**(cfg or {})).cuda().train()
    m.train_impl = impl
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)
    s = (LRWarmupScheduler(torch.optim.lr_scheduler.StepLR(opt, 2, 0.8), epoch_len=4, warmup_t=8, warmup_mode="auto",
                           warmup_factor=1e-4)       # the reference's warm-up (config/default.py)
         if sched else None)
    conf = TR.default_config()
    conf.update({k: v for k, v in (cfg or {}).items() if k in ("scale_factor", "seqsCnt")})
    return m, opt, s, conf


def _batches(n, B, cfg=None, seed=7):
    T = (cfg or {}).get("seqsCnt", 1)
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(B, 3 * T, 4, 4, generator=g) * 8).cuda(), (torch.rand(B, 1, 100, 100, generator=g) * 250).cuda())
            for _ in range(n)]


def _run(step, sched, batches, start=0, on_step=None):
    """Drive `step` over `batches` the reference's way: iter_update after every step, epoch_update every 4."""
    losses = []
    for i, b in enumerate(batches, start):
        losses.append(step(b)["total_loss"].detach().clone())
        if sched is not None:
            sched.iter_update()
            if (i + 1) % 4 == 0:
                sched.epoch_update()
        if on_step is not None:
            on_step(i)
    return losses


def _plain(m, opt, conf):
    return lambda b: TR.train_one_iter(m, opt, b, conf)


def _assert_same_state(ma, oa, mb, ob):
    for (n, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a, b), n
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]), n
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    for (n, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):       # running mean / var, num_batches_tracked
        assert torch.equal(a, b), n


@torch.no_grad()
def _eval(m, x):
    m.eval()
    y = m(x)
    m.train()
    return y


@pytest.mark.parametrize("impl,cfg,B", [("fp16x3", None, 32), ("bf16", None, 32), ("fp16x3", SEQS, 2)],
                         ids=["fp16x3_b32", "bf16_b32", "seqs_T8_sf25_b2"])
def test_graphed_trajectory_is_bit_identical_to_plain(impl, cfg, B):
    batches = _batches(12, B, cfg)
    x_eval = batches[0][0][:2]
    # control: two plain runs agree, so a difference below is the graph's
    ma, oa, sa, conf = _setup(impl, cfg)
    mb, ob, sb, _ = _setup(impl, cfg)
    evals_a, evals_g = [], []
    la = _run(_plain(ma, oa, conf), sa, batches, on_step=lambda i: i == 5 and evals_a.append(_eval(ma, x_eval)))
    lb = _run(_plain(mb, ob, conf), sb, batches)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    _assert_same_state(ma, oa, mb, ob)
    lrs = []
    # graphed: warm-up 1 eager step, then capture + replay; lr follows the warm-up table, then StepLR
    mg, og, sg, _ = _setup(impl, cfg)
    gstep = GraphedTrainStep(mg, og, conf, warmup=1)

    def probe(i):
        lrs.append(og.param_groups[0]["lr"])
        if i == 5:       # an eval forward in the middle: the replays after it must invalidate its weight packs
            evals_g.append(_eval(mg, x_eval))
    lg = _run(gstep, sg, batches, on_step=probe)
    assert gstep.captures == 1
    assert len(set(lrs)) >= 8, lrs
    for i, (x, y) in enumerate(zip(la, lg)):
        assert torch.equal(x, y), (i, float(x), float(y))
    _assert_same_state(ma, oa, mg, og)
    assert float(og.state[next(mg.parameters())]["step"]) == 12
    # eval after graphed training: the same output as the plain-trained model's
    assert torch.equal(evals_a[0], evals_g[0])
    assert torch.equal(_eval(ma, x_eval), _eval(mg, x_eval))


def test_checkpoint_of_graphed_training_resumes_exactly(tmp_path):
    from tactilesr_amd.train.checkpoint import save_checkpoint, load_checkpoint
    batches = _batches(12, 32, seed=11)
    m12, o12, s12, conf = _setup()
    _run(GraphedTrainStep(m12, o12, conf), s12, batches)
    m6, o6, s6, _ = _setup()
    _run(GraphedTrainStep(m6, o6, conf), s6, batches[:6])
    path = str(tmp_path / "ck.pth")
    save_checkpoint(path, m6, o6, s6, epoch=0)
    mr, orr, sr, _ = _setup(seed=3)
    load_checkpoint(path, mr, orr, sr, num_gpus=1)
    _run(_plain(mr, orr, conf), sr, batches[6:], start=6)
    _assert_same_state(m12, o12, mr, orr)


def test_recapture_on_changed_constants_and_refusals():
    batches = _batches(10, 32, seed=5)
    mp, op, _, conf = _setup(sched=False)
    mg, og, _, _ = _setup(sched=False)
    gstep = GraphedTrainStep(mg, og, conf, warmup=1)
    captures = []
    for i, b in enumerate(batches):
        if i == 4:
            for o in (op, og):
                o.param_groups[0]["weight_decay"] = 2e-2
        if i == 7:
            mp.train_impl = mg.train_impl = "bf16"
        lp = TR.train_one_iter(mp, op, b, conf)["total_loss"]
        lg = gstep(b)["total_loss"]
        assert torch.equal(lp, lg), i
        captures.append(gstep.captures)
    # call 2 captures; a changed constant drops the graph: one eager step, then a new capture
    assert captures == [0, 1, 1, 1, 1, 2, 2, 2, 3, 3], captures
    _assert_same_state(mp, op, mg, og)

    x, hr = batches[0]
    with pytest.raises(_lib.TactileSRHipError, match="shape"):
        gstep((x[:16], hr[:16]))
    with pytest.raises(_lib.TactileSRHipError, match="dtype"):
        gstep((x.double(), hr))
    mg.eval()
    with pytest.raises(_lib.TactileSRHipError, match="eval mode"):
        gstep(batches[0])
    mg.train()
    eng = mg.train_engine()
    eng.profile = {}
    with pytest.raises(_lib.TactileSRHipError, match="profile"):
        gstep(batches[0])
    eng.profile = None
    ddp.GradSync(mg)
    with pytest.raises(_lib.TactileSRHipError, match="GradSync"):
        gstep(batches[0])
    eng.grad_sync = eng.arena.on_bucket_ready = None
    with pytest.raises(_lib.TactileSRHipError, match="optim.Adam"):
        GraphedTrainStep(mg, torch.optim.Adam(mg.parameters(), lr=1e-3), conf)
    captures_before = gstep.captures
    gstep(batches[1])                        # still usable after the refusals
    assert gstep.captures == captures_before


def test_graphed_train_step_latency_b32():
    """Prints plain vs graphed ms/step at the reference's train batch; asserts only graphed <= 1.1 x plain."""
    batches = _batches(2, 32, seed=9)
    mp, op, _, conf = _setup(sched=False)
    mg, og, _, _ = _setup(sched=False)
    gstep = GraphedTrainStep(mg, og, conf)
    plain = _plain(mp, op, conf)

    def ms(fn, n=30):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fn(batches[i & 1])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for _ in range(3):
        plain(batches[0])
        gstep(batches[0])
    t = {"plain": [], "graphed": []}
    for _ in range(2):                       # A/B/A/B in one process
        t["plain"].append(ms(plain))
        t["graphed"].append(ms(gstep))
    tp, tg = min(t["plain"]), min(t["graphed"])
    print(f"[train graph] B=32 train step: plain {tp:.3f} ms, graphed {tg:.3f} ms ({tp / tg:.2f}x)")
    assert tg <= 1.1 * tp
