"""Writes tests/golden/ssim.npz: what the reference's own SSIM code (utility/tools.py: calculationSSIM :66-81 and the
"# ssim loss" module SSIM :84-114) gives on two 24x24 pairs, in fp32 and fp64, and the fp64 autograd gradient of the
module with respect to its first argument.

Runs only where a checkout of the reference is present (it imports the reference's utility.tools; nothing of it is
copied: the fixture holds inputs and the reference's outputs).  Not run by the test-suite.

    python tests/golden/make_golden_ssim.py <path of the reference checkout>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    raise SystemExit(__doc__)
sys.path.insert(0, sys.argv[1])

from utility.tools import SSIM, calculationSSIM  # noqa: E402  (reference)

import _ssim_cases as SC  # noqa: E402


def main():
    out = {}
    pairs = [SC.make_pair(1, 24, 24, law, seed) for law, seed in (("clamped", 2401), ("signed", 2402))]
    y = torch.cat([p[0] for p in pairs])[:, 0]          # (2,24,24) fp32
    t = torch.cat([p[1] for p in pairs])[:, 0]
    out["y"], out["t"] = y.numpy(), t.numpy()
    mod = SSIM()
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        out[f"calc_{tag}"] = np.array([float(calculationSSIM(y[i].to(dt), t[i].to(dt))) for i in range(2)], dtype=np.float64)
        out[f"module_{tag}"] = np.array([float(mod(y[i].to(dt), t[i].to(dt))) for i in range(2)], dtype=np.float64)
    grads = []
    for i in range(2):
        yi = y[i].double().clone().requires_grad_(True)
        mod(yi, t[i].double()).backward()
        grads.append(yi.grad.numpy())
    out["grad_f64"] = np.stack(grads)
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
