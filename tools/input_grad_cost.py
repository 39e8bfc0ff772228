#!/usr/bin/env python3
"""Added cost of the taxel gradient (``LR.requires_grad_()``) on the train step: forward + MSE + backward + Adam, timed
with HIP events, with and without ``x.requires_grad`` on the same seeded model and batch, alternated in one process:
    python tools/input_grad_cost.py [--steps N] [--rounds R] [--only NAME]
Configurations: fp16x3 at B = 32 and B = 8192, bf16 at B = 8192 (T = 1, 4x4 -> 40x40), and the Seqs shape (T = 8, sf 25,
4x4x24 -> 100x100) at B = 256.  Prints one line per configuration with the best round of each form and the delta.  The new
kernel's own time comes from a separate profiled run:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/input_grad_cost.py --steps 2 --rounds 1"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tactilesr_amd  # noqa: E402
from tactilesr_amd import optim  # noqa: E402

CONFIGS = (("fp16x3_b32", "fp16x3", 32, {}), ("fp16x3_b8192", "fp16x3", 8192, {}), ("bf16_b8192", "bf16", 8192, {}),
           ("seqs_fp16x3_b256", "fp16x3", 256, dict(scale_factor=25, seqsCnt=8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run only the configuration with this name")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_cost: needs a ROCm device (the timing is of the GPU step)")
    for name, impl, B, cfg in CONFIGS:
        if a.only and name != a.only:
            continue
        sf, T = cfg.get("scale_factor", 10), cfg.get("seqsCnt", 1)
        torch.manual_seed(42)
        m = tactilesr_amd.TactileSR(**cfg).cuda().train()
        m.train_impl = impl
        opt = optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-2)
        g = torch.Generator().manual_seed(43)
        LR = (torch.rand(B, 3 * T, 4, 4, generator=g) * 8).cuda()
        HR = (torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25).cuda()

        def step(with_dx):
            x = LR.detach().requires_grad_(with_dx)
            opt.zero_grad()
            F.mse_loss(m(x), HR).backward()
            opt.step()

        def timed(with_dx):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(with_dx)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps

        for _ in range(a.warmup):
            step(False)
            step(True)
        t = {False: [], True: []}
        for _ in range(a.rounds):
            for k in (False, True):
                t[k].append(timed(k))
        t0, t1 = min(t[False]), min(t[True])
        print(f"[input grad cost] {name} (T={T} sf={sf} B={B} {impl}): without {t0:.3f} ms/step, with {t1:.3f} ms/step, "
              f"delta {t1 - t0:+.3f} ms ({(t1 - t0) / t0 * 100:+.2f} %); rounds without "
              f"{['%.3f' % v for v in t[False]]}, with {['%.3f' % v for v in t[True]]}", flush=True)
        del m, opt, LR, HR
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
