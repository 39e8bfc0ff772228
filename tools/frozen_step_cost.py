#!/usr/bin/env python3
"""Cost of the train step (forward + MSE + backward + Adam) when part of the model is frozen, timed with HIP events:
    python tools/frozen_step_cost.py [--steps N] [--rounds R] [--only NAME] [--out profiles/frozen_step_cost.json]
Crosses
  patterns     all    every parameter trains
               trunk  the Seqs recipe with ``model_param_init(..., freeze=True)``: the MSRBs and ResBlocks are transplanted
                      and frozen, stems / fuse conv / head train (the optimizer is built before the transplant)
               head   only ``output_layer.*`` trains
  arithmetics  ``train_impl`` fp16x3 and bf16
  shapes       sf 10 / T 1 at B = 2048 and B = 32, sf 25 / T 8 at B = 256.
Every (shape, arithmetic) holds one model per pattern, built from the same seed; every model is warmed, then the patterns
alternate inside each of R rounds of N steps.  Reported per pattern: the median round and the spread (max - min) in ms per
step, the ratio to ``all`` of the same run, and whether it is slower than ``all`` by more than the run's spread.

A dead network clocks differently (all-zero activations), so the steps run at the reference's warm-up start learning rate
(lr 1e-3 x warmup_factor 1e-4) and every case prints the fraction of non-zero outputs and the gradient norm of its last
step; a case whose output is all zero is marked invalid.

``--hold-bn`` runs ANOTHER measurement instead and adds it to the same file under the key ``hold_bn`` (the ``cases`` above
stay as they are): the Seqs step (sf 25 / T 8 at B = 256) in both arithmetics with every parameter trainable, with
``model_param_init(freeze=True)`` and with ``model_param_init(freeze=True, hold_bn=True)`` -- the same alternating rounds,
plus the entry-point calls of one step (forward statistics launches, backward BatchNorm launches, all calls)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import tactilesr_amd  # noqa: E402
from tactilesr_amd import optim  # noqa: E402
from tactilesr_amd.train.checkpoint import model_param_init  # noqa: E402

SHAPES = (("sf10_T1_b2048", {}, 2048), ("sf10_T1_b32", {}, 32), ("sf25_T8_b256", dict(scale_factor=25, seqsCnt=8), 256))
IMPLS = ("fp16x3", "bf16")
PATTERNS = ("all", "trunk", "head")
LR_START = 1e-3 * 1e-4          # the reference's base lr x its warm-up factor: the first iteration's learning rate


def build(pattern, cfg, impl):
    torch.manual_seed(42)
    m = tactilesr_amd.TactileSR(**cfg).cuda().train()
    m.train_impl = impl
    opt = optim.Adam(m.parameters(), lr=LR_START, weight_decay=1e-2)
    if pattern == "trunk":
        single_cfg = dict(cfg, seqsCnt=1)
        torch.manual_seed(41)
        sd = tactilesr_amd.TactileSR(**single_cfg).state_dict()
        model_param_init(m, sd, lambda: tactilesr_amd.TactileSR(**single_cfg), freeze=True)
        m.train()
    elif pattern == "head":
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith("output_layer."))
    return m, opt


HOLD_PATTERNS = ("all", "freeze", "freeze_hold_bn")


def build_hold(pattern, cfg, impl):
    torch.manual_seed(42)
    m = tactilesr_amd.TactileSR(**cfg).cuda().train()
    m.train_impl = impl
    opt = optim.Adam(m.parameters(), lr=LR_START, weight_decay=1e-2)
    if pattern != "all":
        single_cfg = dict(cfg, seqsCnt=1)
        torch.manual_seed(41)
        sd = tactilesr_amd.TactileSR(**single_cfg).state_dict()
        model_param_init(m, sd, lambda: tactilesr_amd.TactileSR(**single_cfg), freeze=True, hold_bn=(pattern == "freeze_hold_bn"))
        m.train()          # the trainer's per-epoch model.train(): held layers stay held
    return m, opt


def count_calls(step):
    """Entry-point calls of one step, by name (tsr_conv2d_ex launches under "tsr_conv2d_ex")."""
    from collections import Counter
    from tactilesr_amd.model import _train
    names = Counter()
    call, conv_ex = _train.call, _train.conv_ex

    def call_(name, *args):
        names[name] += 1
        return call(name, *args)

    def conv_ex_(**kw):
        names["tsr_conv2d_ex"] += 1
        return conv_ex(**kw)

    _train.call, _train.conv_ex = call_, conv_ex_
    try:
        step()
    finally:
        _train.call, _train.conv_ex = call, conv_ex
    fam = lambda *pre: sum(v for k, v in names.items() if k.startswith(pre))
    return dict(all_calls=sum(names.values()), conv_ex=names["tsr_conv2d_ex"],
                fwd_stats=fam("tsr_bn_stats_finalize", "tsr_cb16_stats"), bn_eval_vectors=fam("tsr_bn_eval_vectors"),
                bn_bwd_finalize=fam("tsr_bn_bwd_finalize"), bn_bwd_apply=fam("tsr_bn_bwd_apply") - fam("tsr_bn_bwd_apply_eval"),
                bn_bwd_apply_eval=fam("tsr_bn_bwd_apply_eval"))


def hold_bn_main(a):
    shape, cfg, B = SHAPES[2]
    sf, T = cfg["scale_factor"], cfg["seqsCnt"]
    g = torch.Generator().manual_seed(43)
    LR = (torch.rand(B, 3 * T, 4, 4, generator=g) * 8).cuda()
    HR = (torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25).cuda()
    cases = []
    for impl in IMPLS:
        models = {p: build_hold(p, cfg, impl) for p in HOLD_PATTERNS}

        def step(p):
            m, opt = models[p]
            out = m(LR)
            loss = F.mse_loss(out, HR)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return out

        def timed(p):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(p)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps

        for p in HOLD_PATTERNS:
            for _ in range(a.warmup):
                step(p)
        t = {p: [] for p in HOLD_PATTERNS}
        for _ in range(a.rounds):
            for p in HOLD_PATTERNS:
                t[p].append(timed(p))
        med = {p: statistics.median(v) for p, v in t.items()}
        spread = {p: max(v) - min(v) for p, v in t.items()}
        for p in HOLD_PATTERNS:
            m, _ = models[p]
            calls = count_calls(lambda: step(p))
            out = step(p)
            frac = float((out > 0).float().mean())
            case = dict(shape=shape, scale_factor=sf, seqsCnt=T, B=B, train_impl=impl, config=p,
                        ms_per_step_median=round(med[p], 4), ms_per_step_spread=round(spread[p], 4),
                        rounds_ms=[round(v, 4) for v in t[p]], ratio_to_freeze=round(med[p] / med["freeze"], 4),
                        run_spread_ms=round(max(spread.values()), 4), calls=calls, out_nonzero_frac=round(frac, 5),
                        valid=bool(frac > 0))
            cases.append(case)
            print(f"[hold bn step cost] {shape} {impl} {p:14s}: {med[p]:9.3f} ms/step (spread {spread[p]:.3f}), "
                  f"x{case['ratio_to_freeze']:.4f} of freeze; calls {calls}; out_nonzero_frac {frac:.4f}"
                  + ("" if case["valid"] else "  INVALID: the output is all zero"), flush=True)
        del models
        torch.cuda.empty_cache()
    result = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            result = json.load(f)
    result["hold_bn"] = dict(device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds, warmup=a.warmup, lr=LR_START,
                             cases=cases)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"[hold bn step cost] wrote {a.out} (key hold_bn)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run only the shape with this name")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frozen_step_cost.json"))
    ap.add_argument("--hold-bn", action="store_true", help="measure the Seqs step with held BatchNorm statistics instead "
                    "(all trainable / freeze / freeze + hold_bn); added to --out under the key hold_bn")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_step_cost: needs a ROCm device (the timing is of the GPU step)")
    if a.hold_bn:
        return hold_bn_main(a)
    cases = []
    for shape, cfg, B in SHAPES:
        if a.only and shape != a.only:
            continue
        sf, T = cfg.get("scale_factor", 10), cfg.get("seqsCnt", 1)
        g = torch.Generator().manual_seed(43)
        LR = (torch.rand(B, 3 * T, 4, 4, generator=g) * 8).cuda()
        HR = (torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25).cuda()
        for impl in IMPLS:
            models = {p: build(p, cfg, impl) for p in PATTERNS}

            def step(p):
                m, opt = models[p]
                out = m(LR)
                loss = F.mse_loss(out, HR)
                opt.zero_grad()
                loss.backward()
                opt.step()
                return out

            def timed(p):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    step(p)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / a.steps

            for p in PATTERNS:
                for _ in range(a.warmup):
                    step(p)
            t = {p: [] for p in PATTERNS}
            for _ in range(a.rounds):
                for p in PATTERNS:
                    t[p].append(timed(p))
            spread = {p: max(v) - min(v) for p, v in t.items()}
            med = {p: statistics.median(v) for p, v in t.items()}
            run_spread = max(spread.values())
            for p in PATTERNS:
                m, _ = models[p]
                out = step(p)
                frac = float((out > 0).float().mean())
                grads = [q.grad for q in m.parameters() if q.requires_grad and q.grad is not None]
                gnorm = float(torch.nn.utils.get_total_norm(grads))
                case = dict(shape=shape, scale_factor=sf, seqsCnt=T, B=B, train_impl=impl, pattern=p,
                            trainable_tensors=len(grads), ms_per_step_median=round(med[p], 4),
                            ms_per_step_spread=round(spread[p], 4), rounds_ms=[round(v, 4) for v in t[p]],
                            ratio_to_all=round(med[p] / med["all"], 4), run_spread_ms=round(run_spread, 4),
                            slower_than_all_beyond_spread=bool(med[p] - med["all"] > run_spread),
                            out_nonzero_frac=round(frac, 5), grad_norm=gnorm, valid=bool(frac > 0))
                cases.append(case)
                print(f"[frozen step cost] {shape} {impl} {p:5s}: {med[p]:9.3f} ms/step (spread {spread[p]:.3f}), "
                      f"x{case['ratio_to_all']:.3f} of all; out_nonzero_frac {frac:.4f}, grad norm {gnorm:.4e}"
                      + ("" if case["valid"] else "  INVALID: the output is all zero")
                      + ("  SLOWER than all beyond the spread" if case["slower_than_all_beyond_spread"] else ""), flush=True)
            del models
            torch.cuda.empty_cache()
    result = dict(tool="tools/frozen_step_cost.py", device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds,
                  warmup=a.warmup, lr=LR_START, cases=cases)
    if os.path.exists(a.out):          # a --hold-bn measurement already in the file stays
        with open(a.out) as f:
            kept = json.load(f).get("hold_bn")
        if kept is not None:
            result["hold_bn"] = kept
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"[frozen step cost] wrote {a.out}")


if __name__ == "__main__":
    main()
