"""Writes tests/golden/augment.npz: what the reference's own augmentData (utility/raw_data_process.py:57-95) makes of a
seeded 5-sample set of (LR (3,4,4), depth (100,100)) pairs -- the inputs and the 20 samples it returns, in its order.

Runs only where a checkout of the reference is present (it imports the reference's utility.raw_data_process; nothing of
it is copied: the fixture holds inputs and the reference's outputs).  Not run by the test-suite.  The reference module
imports cv2 at its top, which augmentData never uses: where cv2 is not installed an empty stand-in module is registered
under that name before the import.

    python tests/golden/make_golden_augment.py <path of the reference checkout>
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    raise SystemExit(__doc__)
sys.path.insert(0, sys.argv[1])
if importlib.util.find_spec("cv2") is None:
    sys.modules["cv2"] = types.ModuleType("cv2")

from utility.raw_data_process import augmentData  # noqa: E402  (reference)


def main():
    rng = np.random.default_rng(5701)
    LR = rng.standard_normal((5, 3, 4, 4)).astype(np.float32)
    depth = rng.integers(0, 16, (5, 100, 100)).astype(np.float32)      # 16 levels: the fixture compresses to ~210 KB
    aug = augmentData([{"LR": LR[i], "depth": depth[i]} for i in range(5)])
    out = dict(LR=LR, depth=depth, aug_LR=np.stack([np.asarray(d["LR"]) for d in aug]),
               aug_depth=np.stack([np.asarray(d["depth"]) for d in aug]))
    assert out["aug_LR"].shape == (20, 3, 4, 4) and out["aug_depth"].shape == (20, 100, 100)
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
