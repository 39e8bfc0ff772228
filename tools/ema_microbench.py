#!/usr/bin/env python3
"""Cost of the weight-averaging launch (tsr_ema_multi), timed with HIP events:
    python tools/ema_microbench.py [--rounds R] [--only update|step] [--out profiles/ema_cost.json]
Measures, on the full default model (124 parameter tensors + 27 x 3 BatchNorm buffers, 4.59 M elements)
  update   one averaging update, warm-up schedule, buffers copied: ``WeightEMA.update()`` (the cached-table lookup and the
           launch), the bare ``tsr_ema_multi`` launch on that table, and the same update composed from torch ops
           (``torch._foreach_lerp_`` over the parameters, ``torch._foreach_copy_`` over the buffers) -- what a user has
           without the kernel.  Per call: ms between device events over back-to-back calls, the host time to enqueue one
           call (no synchronise inside the window), and the HBM bytes the update has to move over the event time.
  step     the train step at B = 32 (train_impl fp16x3, sf 10 / T 1): ``GraphedTrainStep`` without and with ``ema``, and
           eager ``train_one_iter`` without an average, with ``ema`` and with the torch composition after the step.
Every configuration of one comparison holds its own model from the same seed; all are warmed, then they alternate inside
each of R rounds; reported are the median round and the spread (max - min) in ms, and for the steps the difference to the
step without an average.  Steps run at the reference's warm-up start learning rate on contact-like blob targets.  A run
without a ROCm device fails: nothing here is estimated."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import tactilesr_amd  # noqa: E402
from tactilesr_amd import _lib, optim  # noqa: E402
from tactilesr_amd.ema import UPDATE, WeightEMA  # noqa: E402
from tactilesr_amd.train import tactileSR_train as TR  # noqa: E402
from tactilesr_amd.train.graph import GraphedTrainStep  # noqa: E402

LR_START = 1e-3 * 1e-4          # the reference's base lr x its warm-up factor: the first iteration's learning rate
DECAY, WARMUP = 0.999, 10


def blobs(B, H, W, gen, amp=10.0):
    """(B,1,H,W): three Gaussian blobs per image, the largest pixel at most `amp`."""
    r = torch.arange(H, dtype=torch.float32)[None, :, None]
    c = torch.arange(W, dtype=torch.float32)[None, None, :]
    img = torch.zeros(B, H, W)
    for _ in range(3):
        a = 2 + 8 * torch.rand(B, 1, 1, generator=gen)
        cr, cc = torch.rand(B, 1, 1, generator=gen) * H, torch.rand(B, 1, 1, generator=gen) * W
        s = (0.04 + 0.08 * torch.rand(B, 1, 1, generator=gen)) * max(H, W)
        img = img + a * torch.exp(-((r - cr) ** 2 + (c - cc) ** 2) / (2 * s * s))
    return (img * (amp / img.amax(dim=(1, 2), keepdim=True).clamp_min(amp)))[:, None].contiguous()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def enqueue_us(fn, n):
    """Host time of one call, the device left to drain afterwards (outside the window)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t = (time.perf_counter() - t0) / n * 1e6
    torch.cuda.synchronize()
    return t


def alternate(fns, warmup, rounds, n):
    """{name: [ms per call, one per round]}: every fn warmed, then the fns take turns inside each round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, n))
    return t


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 5), "ms_spread": round(max(ms) - min(ms), 5),
            "rounds_ms": [round(v, 5) for v in ms]}


class TorchComposed:
    """The same update from torch ops: a lerp over the parameters and a copy over the buffers, on shadows of its own."""

    def __init__(self, model):
        self.params = [p.detach() for p in model.parameters()]
        self.bufs = [b for b in model.buffers()]
        self.sp = [p.clone() for p in self.params]
        self.sb = [b.clone() for b in self.bufs]
        self.t = 0

    def update(self):
        decay = min(DECAY, (1 + self.t) / (WARMUP + self.t))
        torch._foreach_lerp_(self.sp, self.params, 1.0 - decay)
        torch._foreach_copy_(self.sb, self.bufs)
        self.t += 1


def model(seed=42):
    torch.manual_seed(seed)
    return tactilesr_amd.TactileSR().cuda().train()


def update_cases(a):
    m = model()
    e = WeightEMA(m, decay=DECAY, warmup=WARMUP)
    e.update()
    table, n_chunks = e._table(e._live())
    tc = TorchComposed(m)
    lib, tp, omd = _lib.load(), ctypes.c_void_p(table.data_ptr()), ctypes.c_float(1e-3)

    def bare():
        lib.tsr_ema_multi(tp, ctypes.c_int(n_chunks), ctypes.c_int(UPDATE), omd, _lib.stream())

    fns = {"ema_update": e.update, "ema_launch_alone": bare, "torch_foreach_lerp_copy": tc.update}
    rounds = alternate(fns, a.warmup, a.rounds, a.launches)
    n_par = sum(p.numel() for p in m.parameters())
    buf_bytes = sum(b.numel() * b.element_size() for b in m.buffers())
    moved = 3 * 4 * n_par + 2 * buf_bytes               # read avg and src, write avg; buffers: read src, write avg
    base = statistics.median(rounds["torch_foreach_lerp_copy"])
    out = []
    for k, ms in rounds.items():
        s = summary(ms)
        s.update({"call": k, "host_enqueue_us": round(enqueue_us(fns[k], a.launches), 2),
                  "ratio_to_torch_composed": round(s["ms_median"] / base, 3), "bytes_moved": moved,
                  "gb_per_s": round(moved / s["ms_median"] / 1e6, 1)})
        out.append(s)
        print(f"[update] {k:26s} {s['ms_median']:.5f} ms (spread {s['ms_spread']:.5f}), host enqueue "
              f"{s['host_enqueue_us']:.1f} us, {s['gb_per_s']:.0f} GB/s", flush=True)
    return {"tensors": {"parameters": len(list(m.parameters())), "buffers": len(list(m.buffers()))},
            "elements": n_par, "records": n_chunks, "calls": out}


def step_cases(a, B=32):
    conf = dict(TR.default_config())
    gen = torch.Generator().manual_seed(43)
    batch = ((torch.rand(B, 3, 4, 4, generator=gen) * 8).cuda(), (blobs(B, 100, 100, gen, amp=100.0)).cuda())

    def make(kind):
        m = model()
        o = optim.Adam(m.parameters(), lr=LR_START, weight_decay=1e-2)
        if kind == "graph":
            g = GraphedTrainStep(m, o, conf, warmup=1)
            return lambda: g(batch)
        if kind == "graph_ema":
            g = GraphedTrainStep(m, o, conf, warmup=1, ema=WeightEMA(m, decay=DECAY, warmup=WARMUP))
            return lambda: g(batch)
        if kind == "eager":
            return lambda: TR.train_one_iter(m, o, batch, conf)
        if kind == "eager_ema":
            e = WeightEMA(m, decay=DECAY, warmup=WARMUP)
            return lambda: TR.train_one_iter(m, o, batch, conf, ema=e)
        tc = TorchComposed(m)

        def step():
            TR.train_one_iter(m, o, batch, conf)
            tc.update()
        return step

    fns = {k: make(k) for k in ("graph", "graph_ema", "eager", "eager_ema", "eager_torch_composed")}
    rounds = alternate(fns, max(a.warmup, 3), a.rounds, a.steps)
    out = []
    for k, ms in rounds.items():
        s = summary(ms)
        ref = statistics.median(rounds["graph" if k.startswith("graph") else "eager"])
        s.update({"step": k, "batch": B, "ms_over_no_average": round(s["ms_median"] - ref, 5)})
        out.append(s)
        print(f"[step B={B}] {k:22s} {s['ms_median']:.4f} ms (spread {s['ms_spread']:.4f}), "
              f"{s['ms_over_no_average']:+.4f} ms over the step without an average", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200, help="update calls per timed window")
    ap.add_argument("--steps", type=int, default=30, help="train steps per timed window")
    ap.add_argument("--only", choices=("update", "step"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ema_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_microbench needs a ROCm device: nothing is estimated without one")
    res = {"tool": "tools/ema_microbench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "warmup": a.warmup, "launches": a.launches, "steps": a.steps, "decay": DECAY, "decay_warmup": WARMUP}
    if a.only != "step":
        res["update"] = update_cases(a)
    if a.only != "update":
        res["step_b32"] = step_cases(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
