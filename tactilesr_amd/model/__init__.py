from .tactileSR_model import TactileSR, TactileSRCNN, MSRB, ResBlock, hold_bn_statistics  # noqa: F401
