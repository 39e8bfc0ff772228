"""tactilesr_amd: MI355X-native (gfx950) implementation of the tactileSR hot path --
the TactileSR conv upscaler and the tPSFNet PSF forward model -- behind the reference's
own model interface.  Host code is Python on PyTorch-ROCm; every hot op is a hand-written
HIP kernel in ``lib/libtactilesr_hip.so`` reached through the C ABI of
``include/tactilesr_hip.h``.  No CPU fallback exists in this package.
"""
from . import _lib  # noqa: F401
from .model.tactileSR_model import TactileSR, TactileSRCNN, MSRB, ResBlock  # noqa: F401
from .model.tPSFNet import tPSFNet  # noqa: F401
from .ema import WeightEMA, recalibrate_bn  # noqa: F401


def invalidate_weight_packs() -> None:
    """Drop every cached weight pack and eval plan of every module of this package: the next eval forward packs again.
    Call it after a write the caches cannot see -- an in-place edit through ``.data`` (``p.data.mul_(2)``,
    ``p.data.clamp_(..)``) leaves both the tensor's address and its version counter as they were.  Every other writer
    (in-place under ``no_grad``, ``load_state_dict``, optimizers, ``WeightEMA``, the train step) is seen without it."""
    _lib.bump_param_epoch()


__all__ = ["TactileSR", "TactileSRCNN", "MSRB", "ResBlock", "tPSFNet", "WeightEMA", "recalibrate_bn",
           "invalidate_weight_packs"]
