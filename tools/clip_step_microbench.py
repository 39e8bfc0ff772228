#!/usr/bin/env python3
"""What gradient-norm clipping costs in the train step at B = 32 (T = 1, 4x4 -> 40x40):
    python tools/clip_step_microbench.py [--steps N] [--rounds R] [--impl fp16x3|bf16] [--clip C]
Five forms on the same seeded model and batch: the plain ``train_one_iter``; the reference's recipe (torch's
``clip_grad_norm_`` over ``model.parameters()``, then ``optim.Adam.step``); the fused ``train_one_iter(...,
clip_grad_norm=C)`` (``Adam.step_clipped``); and ``GraphedTrainStep`` without and with clipping.  Warm-up first, then R
rounds of all forms in turn (one process), N steps each, a host clock that ends in torch.cuda.synchronize(); the best
round of each form is printed.  A second table times the optimizer call alone on the gradients of one backward: plain
``step()``, ``clip_grad_norm_`` + ``step()``, ``step_clipped``."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tactilesr_amd  # noqa: E402
from tactilesr_amd import optim  # noqa: E402
from tactilesr_amd.train import tactileSR_train as TR  # noqa: E402
from tactilesr_amd.train.graph import GraphedTrainStep  # noqa: E402


def make(impl):
    torch.manual_seed(42)
    m = tactilesr_amd.TactileSR().cuda().train()
    m.train_impl = impl
    return m, optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)


def ms_per_call(fn, arg, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--impl", default="fp16x3")
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    conf = TR.default_config()
    g = torch.Generator().manual_seed(42)
    B = a.batch
    batch = ((torch.rand(B, 3, 4, 4, generator=g) * 8).cuda(), (torch.rand(B, 1, 100, 100, generator=g) * 250).cuda())
    c = a.clip

    def recipe(m, opt):
        def step(b):
            losses, loss_dict = TR.train_cal_loss(m, b, conf)
            opt.zero_grad()
            losses.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), c)
            opt.step()
            return loss_dict
        return step

    models = {k: make(a.impl) for k in ("plain", "recipe", "fused", "graphed", "graphed_clip")}
    forms = {
        "plain": (lambda m, o: lambda b: TR.train_one_iter(m, o, b, conf))(*models["plain"]),
        "recipe": recipe(*models["recipe"]),
        "fused": (lambda m, o: lambda b: TR.train_one_iter(m, o, b, conf, clip_grad_norm=c))(*models["fused"]),
        "graphed": GraphedTrainStep(*models["graphed"], conf),
        "graphed_clip": GraphedTrainStep(*models["graphed_clip"], conf, clip_grad_norm=c),
    }
    for fn in forms.values():
        for _ in range(a.warmup):
            fn(batch)
    t = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            t[k].append(ms_per_call(fn, batch, a.steps))
    for k, v in t.items():
        print(f"[clip step] B={B} {a.impl} {k:13s} {min(v):.3f} ms/step (rounds {['%.3f' % x for x in v]})", flush=True)

    # the optimizer call alone, on the gradients of one backward (they stay in place: clipping again is idempotent
    # for the fused form only up to rounding, which does not change the timing)
    m, opt = models["plain"]
    losses, _ = TR.train_cal_loss(m, batch, conf)
    opt.zero_grad()
    losses.backward()
    calls = {"step": lambda _: opt.step(),
             "clip_grad_norm_+step": lambda _: (torch.nn.utils.clip_grad_norm_(m.parameters(), c), opt.step()),
             "step_clipped": lambda _: opt.step_clipped(c)}
    for fn in calls.values():
        fn(None)
    t = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            t[k].append(ms_per_call(fn, None, 10 * a.steps))
    for k, v in t.items():
        print(f"[clip opt]  {k:21s} {min(v) * 1e3:.1f} us/call (rounds {['%.1f' % (x * 1e3) for x in v]})", flush=True)


if __name__ == "__main__":
    main()
