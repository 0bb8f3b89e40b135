"""Automatic white balance (an extension): the settings of the ISP's gray-world loop.

`Camera16/32(auto_white_balance=...)` takes False, True or an AutoWhiteBalance.  Every raw load adds statistics of its
frames to a pending buffer on the device; every update_metering (and ISP.update_white_balance) turns them into gains
that the next loads apply in the raw domain, through the lens shading path.  DESIGN.md 3, "Auto white balance".
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np


@dataclasses.dataclass(frozen=True)
class AutoWhiteBalance:
    """stride: sample every stride-th 2x2 quad in each direction (4: every 8th pixel, as the metering).  clip / floor: a
    quad is kept when all four pre-cast values are below clip and the largest is at least floor (values in [0, 1] units
    of the loader)."""
    stride: int = 4
    clip: float = 0.95
    floor: float = 0.02

    def __post_init__(self):
        if isinstance(self.stride, bool) or not isinstance(self.stride, (int, np.integer)) or self.stride < 1:
            raise ValueError(f"AutoWhiteBalance.stride must be an int >= 1, got {self.stride!r}")
        for name in ("clip", "floor"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"AutoWhiteBalance.{name} must be a finite number, got {v!r}")
        if not 0 < self.floor < self.clip:
            raise ValueError(f"AutoWhiteBalance needs 0 < floor < clip, got floor {self.floor}, clip {self.clip}")


def check_auto_white_balance(value):
    """The AutoWhiteBalance of a constructor / set() argument (True: the defaults), None for False; ValueError otherwise."""
    if value is False:
        return None
    if value is True:
        return AutoWhiteBalance()
    if isinstance(value, AutoWhiteBalance):
        return value
    raise ValueError(f"auto_white_balance must be False, True or an AutoWhiteBalance, got {type(value).__name__}")


def check_seed(white_balance):
    """The seed gains f32(white_balance), (3,); ValueError unless three finite values > 0."""
    wb = np.asarray(white_balance, dtype=np.float64).reshape(-1)
    if wb.size != 3 or not np.all(np.isfinite(wb)) or not np.all(wb > 0):
        raise ValueError(f"white_balance must hold three finite gains > 0 for auto_white_balance, got {white_balance!r}")
    return wb.astype(np.float32)
