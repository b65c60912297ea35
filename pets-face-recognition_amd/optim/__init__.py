from .fused import FusedSGD, FusedAdamW, WeightAverage  # noqa: F401
