from .device_loader import DeviceSRLoader  # noqa: F401,E402
from . import seqs_depth2tactile  # noqa: F401,E402


def augment_arrays(LR, depth):
    """The reference's 4x set (``augmentData``, utility/raw_data_process.py:57-95) materialised, for people who save
    datasets: every ``(LR (C,h,w), depth (H,W))`` sample becomes four in a row -- the original, then ``np.rot90`` by 1, 2
    and 3 quarter turns of each taxel plane and of the depth map.  ``LR`` is ``(N,C,h,w)``, ``depth`` ``(N,H,W)`` (or
    ``(N,C,H,W)``), both with square planes; returns numpy arrays of ``4N`` samples.  Training does not need the copies:
    ``DeviceSRLoader(..., augment="rot90", augment_mode="expand")`` walks the same set in the same order."""
    import numpy as np
    LR, depth = np.asarray(LR), np.asarray(depth)
    assert LR.shape[0] == depth.shape[0], "LR and depth must hold the same number of samples"
    assert LR.shape[-1] == LR.shape[-2] and depth.shape[-1] == depth.shape[-2], "quarter turns need square planes"
    out_LR = np.stack([np.rot90(LR, k, axes=(-2, -1)) for k in range(4)], axis=1)
    out_depth = np.stack([np.rot90(depth, k, axes=(-2, -1)) for k in range(4)], axis=1)
    return (np.ascontiguousarray(out_LR.reshape((-1,) + LR.shape[1:])),
            np.ascontiguousarray(out_depth.reshape((-1,) + depth.shape[1:])))


def tpsf_loader(LR, depth, config, batch_size, **kw) -> DeviceSRLoader:
    """The tPSFNet trainer's loader over ``(LR, depth)`` pairs, honouring ``config["is_aug_data"]`` the way the reference's
    ``tPSFNetDataSet(..., is_aug_data=config['is_aug_data'])`` does (train/tPSFNet_train.py:31-32): set, the loader
    covers every sample under the four quarter turns (``augment="rot90", augment_mode="expand"``, the transform done on
    the device batch by batch); unset or absent, it is the plain loader.  An optional ``config["taxel_noise"]`` (a
    ``functional.TaxelNoise`` or a dict of its fields) and ``config["taxel_noise_seed"]`` become the loader's
    ``taxel_noise`` / ``noise_seed``; absent (or ``None``), the loader is unchanged.  ``kw`` goes to ``DeviceSRLoader`` and
    may override any of these choices."""
    import torch
    if config.get("is_aug_data", False):
        kw = dict(dict(augment="rot90", augment_mode="expand"), **kw)
    if config.get("taxel_noise") is not None:
        kw = dict(dict(taxel_noise=config["taxel_noise"], noise_seed=config.get("taxel_noise_seed")), **kw)
    return DeviceSRLoader(torch.as_tensor(LR), torch.as_tensor(depth), batch_size, **kw)
