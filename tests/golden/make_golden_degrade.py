"""Writes tests/golden/degrade.npz: what the reference's own degradation_process (model/tPSFNet.py:129-141, fp32) gives on
six 100x100 images -- one contact image per gamma in {0.05, 0.7, 5, 50} and a signed one for 0.7 and 5.

Runs only where a checkout of the reference is present (it imports the reference's model.tPSFNet; nothing of it is
copied: the fixture holds inputs, the gammas and the reference's outputs).  Not run by the test-suite.

    python tests/golden/make_golden_degrade.py <path of the reference checkout>
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

from model.tPSFNet import tPSFNet  # noqa: E402  (reference)

import _degrade_cases as DC  # noqa: E402


def main():
    gen = torch.Generator().manual_seed(4100)
    y = torch.cat([DC.blobs(4, 100, 100, gen), DC.blobs(2, 100, 100, gen, signed=True)])      # (6,1,100,100) fp32
    gamma = torch.tensor(list(DC.GAMMAS) + [0.7, 5.0], dtype=torch.float32)
    net = tPSFNet(None, None, device="cpu")
    lr = []
    with torch.no_grad():
        for i in range(y.shape[0]):
            ab = torch.tensor([[1.0, 1.0, float(gamma[i])]], dtype=torch.float32)
            lr.append(net.degradation_process(y[i:i + 1], ab).reshape(16))
    out = {"y": y[:, 0].numpy(), "gamma": gamma.numpy(), "lr_deg_f32": torch.stack(lr).numpy()}
    path = os.path.join(HERE, "degrade.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
