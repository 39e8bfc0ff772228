#!/usr/bin/env python3
"""Host-clock time per training step of the plain ``train_one_iter`` against ``GraphedTrainStep`` (HIP-graph replay of
the whole step), at B = 32 and B = 256 (T = 1, 4x4 -> 40x40) and at the Seqs shape (T = 8, sf 25, 4x4x24 -> 100x100):
    python tools/train_graph_latency.py [--steps N] [--rounds R] [--impl fp16x3|bf16] [--seqs-batch B]
Same seeded model and batch for both forms, warm-up first, then R rounds of plain / graphed (A/B/A/B in one process),
N steps each, a host clock that ends in torch.cuda.synchronize(); the best round of each form is printed, one line
per configuration."""
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


def make(cfg, impl):
    torch.manual_seed(42)
    m = tactilesr_amd.TactileSR(**cfg).cuda().train()
    m.train_impl = impl
    return m, optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-2)


def ms_per_step(fn, batch, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--impl", default="fp16x3")
    ap.add_argument("--seqs-batch", type=int, default=32)
    a = ap.parse_args()
    for name, B, cfg in (("T=1 sf=10", 32, {}), ("T=1 sf=10", 256, {}),
                         ("Seqs T=8 sf=25", a.seqs_batch, dict(scale_factor=25, seqsCnt=8))):
        conf = TR.default_config()
        conf.update(cfg)
        T = cfg.get("seqsCnt", 1)
        g = torch.Generator().manual_seed(42)
        batch = ((torch.rand(B, 3 * T, 4, 4, generator=g) * 8).cuda(), (torch.rand(B, 1, 100, 100, generator=g) * 250).cuda())
        mp, op = make(cfg, a.impl)
        mg, og = make(cfg, a.impl)
        forms = {"plain": lambda b: TR.train_one_iter(mp, op, b, conf), "graphed": GraphedTrainStep(mg, og, conf)}
        for fn in forms.values():
            for _ in range(a.warmup):
                fn(batch)
        t = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                t[k].append(ms_per_step(fn, batch, a.steps))
        tp, tg = min(t["plain"]), min(t["graphed"])
        print(f"[train graph] {name} B={B} {a.impl}: plain {tp:.3f} ms/step, graphed {tg:.3f} ms/step "
              f"({tp / tg:.2f}x; rounds plain {['%.3f' % x for x in t['plain']]}, graphed {['%.3f' % x for x in t['graphed']]})",
              flush=True)
        del forms, mp, op, mg, og
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
