#!/usr/bin/env python3
"""Cost of the fused optimizer launches, timed with HIP events:
    python tools/optim_microbench.py [--rounds R] [--launches N] [--out profiles/optim_cost.json]
On the full default model's table of 124 parameter tensors (4.59 M elements), back to back on one stream:
  adam_l2_multi            the legacy launch (tsr_adam_l2_multi): torch.optim.Adam, what optim.Adam issues
  ex_flags0                the extended launch (tsr_adam_multi_ex) with flags 0: the same formula from the new kernel
  ex_decoupled             ... TSR_ADAM_DECOUPLED: AdamW
  ex_decoupled_amsgrad     ... TSR_ADAM_DECOUPLED | TSR_ADAM_AMSGRAD: two more tensor passes (max_exp_avg_sq read, written)
  ex_decoupled_clip_one    ... DECOUPLED with `clip`, coefficient 1: the gradient is not rewritten (the legacy's bytes)
  ex_decoupled_clip_active ... DECOUPLED with `clip`, coefficient just below 1: one more pass (the gradient written back)
  torch_adamw              torch.optim.AdamW.step() in its default mode on the same tensors
  torch_adamw_fused        torch.optim.AdamW(fused=True).step(), if this torch build has it for ROCm (recorded if not)
Every configuration owns its tensors (clones of the same model and gradients); all are warmed, then they alternate inside
each of R rounds.  Reported per configuration: the median round and the spread (max - min) in ms per call, the bytes the
formula has to move (4 bytes x elements x tensor passes) over that time, and the ratio to the legacy launch of the same
run.  One configuration's working set (7 passes over 18.4 MB) fits the 256 MiB Infinity Cache and the calls of a window
run back to back on it, so the GB/s column is a rate through the cache hierarchy, not an HBM bandwidth; the ratios
between configurations are what the expectation (equal bytes: equal time; AMSGrad: 9/7) is about.  The learning rate is
the reference's warm-up start, so thousands of calls leave the values where they were.  A run without a ROCm device
fails: nothing here is estimated."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import tactilesr_amd  # noqa: E402
from tactilesr_amd import _lib, optim  # noqa: E402

LR_START = 1e-3 * 1e-4          # the reference's base lr x its warm-up factor
BETAS, EPS, WD = (0.9, 0.999), 1e-8, 1e-2
F, I, D = ctypes.c_float, ctypes.c_int, ctypes.c_double


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


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


def tensors(seed=42):
    """Clones of the default model's parameters with gradients of a trained-like magnitude."""
    torch.manual_seed(seed)
    m = tactilesr_amd.TactileSR()
    g = torch.Generator().manual_seed(seed + 1)
    params = [torch.nn.Parameter(p.detach().clone().cuda()) for p in m.parameters()]
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * 1e-3).cuda()
    return params


def launch_case(kind):
    """A bare launch over the chunk table an optimizer of its own built in one eager step."""
    params = tensors()
    ams = kind == "ex_decoupled_amsgrad"
    if kind in ("adam_l2_multi", "ex_flags0"):
        opt = optim.Adam(params, lr=LR_START, betas=BETAS, eps=EPS, weight_decay=WD)
    else:
        opt = optim.AdamW(params, lr=LR_START, betas=BETAS, eps=EPS, weight_decay=WD, amsgrad=ams)
    opt.step()
    (group, step, items), = list(opt._launch_sets(advance=False))
    table = opt._table(items, build=False, vmax=ams)
    lib, tp, n_chunks = _lib.load(), ctypes.c_void_p(table[0].data_ptr()), I(table[1])
    vp = ctypes.c_void_p(table[2].data_ptr() if ams else 0)
    flags = {"ex_flags0": 0, "ex_decoupled_amsgrad": optim.DECOUPLED | optim.AMSGRAD}.get(kind, optim.DECOUPLED)
    coef = {"ex_decoupled_clip_one": 1.0, "ex_decoupled_clip_active": 1.0 - 2.0 ** -20}.get(kind)
    clip = torch.tensor([coef], dtype=torch.float32).cuda() if coef is not None else None
    cp = ctypes.c_void_p(clip.data_ptr() if clip is not None else 0)
    tail = (F(LR_START), D(BETAS[0]), D(BETAS[1]), F(EPS), F(WD), I(step))

    if kind == "adam_l2_multi":
        def fn():
            lib.tsr_adam_l2_multi(tp, n_chunks, *tail, _lib.stream())
    else:
        def fn():
            lib.tsr_adam_multi_ex(tp, vp, n_chunks, I(flags), *tail, cp, _lib.stream())
    passes = 7 + (2 if ams else 0) + (1 if kind == "ex_decoupled_clip_active" else 0)
    return fn, passes, (opt, params, table, clip)          # the last: kept alive with the closure


def torch_case(fused):
    params = tensors()
    kw = dict(fused=True) if fused else {}
    opt = torch.optim.AdamW(params, lr=LR_START, betas=BETAS, eps=EPS, weight_decay=WD, **kw)
    opt.step()
    torch.cuda.synchronize()
    return opt.step, 7, (opt, params)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_microbench needs a ROCm device: nothing is estimated without one")
    fns, passes, keep, notes = {}, {}, [], {}
    for kind in ("adam_l2_multi", "ex_flags0", "ex_decoupled", "ex_decoupled_amsgrad", "ex_decoupled_clip_one",
                 "ex_decoupled_clip_active"):
        fns[kind], passes[kind], k = launch_case(kind)
        keep.append(k)
    for name, fused in (("torch_adamw", False), ("torch_adamw_fused", True)):
        try:
            fns[name], passes[name], k = torch_case(fused)
            keep.append(k)
        except Exception as e:      # a torch build without the fused ROCm kernel says so here
            notes[name] = f"not available in this torch build: {type(e).__name__}: {str(e)[:200]}"
            print(f"[optim] {name}: {notes[name]}", flush=True)
    n_par = sum(p.numel() for p in keep[0][1])
    rounds = alternate(fns, a.warmup, a.rounds, a.launches)
    base = statistics.median(rounds["adam_l2_multi"])
    calls = []
    for k, ms in rounds.items():
        med = statistics.median(ms)
        moved = 4 * n_par * passes[k]
        s = {"call": k, "ms_median": round(med, 5), "ms_spread": round(max(ms) - min(ms), 5),
             "rounds_ms": [round(v, 5) for v in ms], "tensor_passes": passes[k], "bytes_moved": moved,
             "gb_per_s": round(moved / med / 1e6, 1), "ratio_to_adam_l2_multi": round(med / base, 3),
             "expected_ratio_by_bytes": round(passes[k] / 7, 3)}
        calls.append(s)
        print(f"[optim] {k:26s} {s['ms_median']:.5f} ms (spread {s['ms_spread']:.5f}), {s['gb_per_s']:.0f} GB/s, "
              f"x{s['ratio_to_adam_l2_multi']:.3f} of the legacy launch (by bytes: x{s['expected_ratio_by_bytes']:.3f})",
              flush=True)
    res = {"tool": "tools/optim_microbench.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "rounds": a.rounds, "warmup": a.warmup, "launches": a.launches, "tensors": len(keep[0][1]), "elements": n_par,
           "records": keep[0][2][1], "lr": LR_START, "betas": list(BETAS), "eps": EPS, "weight_decay": WD,
           "note": "one configuration's working set fits the 256 MiB Infinity Cache: gb_per_s is not an HBM bandwidth",
           "calls": calls, "unavailable": notes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
