#!/usr/bin/env python3
"""Time tpsf_forward / tpsf_backward alone (HIP events, B samples):  python tools/tpsf_microbench.py [B] [iters] [--grads LIST]

--grads takes a comma-separated subset of hr,psf,depth,x and also times the backward with those paths on: tpsf_backward_ex with
dLR_deg plus an upstream dHR (hr), an upstream dpsf (psf) and the depth gradient (depth), and -- for x -- the one extra GEMM of
the module's backward (layer-0 dy times W0).  `--grads hr,psf,depth,x --each` times every path alone as well."""
import argparse
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tactilesr_amd._lib import call, ptr, stream, c_int as I, c_longlong as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=8192)
ap.add_argument("iters", nargs="?", type=int, default=20)
ap.add_argument("--grads", default="", help="subset of hr,psf,depth,x")
ap.add_argument("--each", action="store_true", help="also time every path of --grads alone")
ap.add_argument("--repeat", type=int, default=1, help="repeat every timing (run-to-run spread)")
args = ap.parse_args()
grads = [g for g in args.grads.split(",") if g]
assert set(grads) <= {"hr", "psf", "depth", "x"}, grads

B, iters = args.B, args.iters
g = torch.Generator().manual_seed(0)
depth = (torch.rand(B, 100, 100, generator=g) * 10).cuda()
ab = (torch.rand(B, 3, generator=g) * 0.5 + 0.7).cuda()
HR = torch.empty(B, 1, 100, 100, device="cuda")
LRd = torch.empty(B, 16, device="cuda")
psf = torch.empty(B, 1, 99, 99, device="cuda")
dl = torch.randn(B, 16, generator=g).cuda()
dab = torch.empty(B, 3, device="cuda")


def timeit(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def times(fn):
    return [timeit(fn) for _ in range(args.repeat)]


def fmt(ts):
    return " ".join(f"{t:.3f}" for t in ts)


work = torch.empty(B * 10000, device="cuda")
fwd = lambda: call("tpsf_forward", ptr(depth), ptr(ab), ptr(HR), ptr(LRd), ptr(psf), I(B), stream())          # noqa: E731
bwd = lambda: call("tpsf_backward", ptr(depth), ptr(ab), ptr(HR), ptr(dl), ptr(dab), ptr(work), I(B), stream())  # noqa: E731
tfs, tbs = times(fwd), times(bwd)
tf, tb = min(tfs), min(tbs)
fb = 4 * (10000 + 10000 + 9801 + 16 + 3)
print(f"tpsf_forward  B={B}: {tf:.3f} ms  {B / tf / 1e3:.2f} M samples/s  {B * fb / tf / 1e6:.0f} GB/s ({B * fb / tf / 8e9 * 100:.1f}% of 8 TB/s)")
print(f"tpsf_backward B={B}: {tb:.3f} ms  {B / tb / 1e3:.2f} M samples/s  {B * 40000 / tb / 1e6:.0f} GB/s")
if args.repeat > 1:
    print(f"tpsf_forward  runs (ms): {fmt(tfs)}")
    print(f"tpsf_backward runs (ms): {fmt(tbs)}")

if grads:
    dHR = (torch.randn(B, 100, 100, generator=g) * 1e-4).cuda()
    dpsf = torch.randn(B, 99, 99, generator=g).cuda()
    dd = torch.empty(B, 100, 100, device="cuda")
    dy0 = torch.randn(B, 256, generator=g).cuda()
    W0 = (torch.randn(256, 48, generator=g) * 0.03).cuda()
    dx = torch.empty(B, 48, device="cuda")

    def run(paths):
        call("tpsf_backward_ex", ptr(depth), ptr(ab), ptr(HR), ptr(dl), ptr(dHR if "hr" in paths else None),
             ptr(dpsf if "psf" in paths else None), ptr(dab), ptr(dd if "depth" in paths else None), ptr(work), I(B), stream())
        if "x" in paths:
            call("tsr_sgemm", ptr(dy0), L(256), L(1), ptr(W0), L(48), L(1), ptr(None), ptr(dx), I(B), I(48), I(256), I(0), stream())

    sets = [grads] + ([[p] for p in grads] if args.each and len(grads) > 1 else [])
    base = times(lambda: run([]))
    print(f"tpsf_backward_ex B={B} dLR_deg only: {min(base):.3f} ms" + (f"  runs: {fmt(base)}" if args.repeat > 1 else ""))
    for paths in sets:
        ts = times(lambda: run(paths))
        print(f"tpsf_backward_ex B={B} dLR_deg + {','.join(paths)}: {min(ts):.3f} ms  (+{min(ts) - min(base):.3f} ms)"
              + (f"  runs: {fmt(ts)}" if args.repeat > 1 else ""))
