"""Green equalisation (an extension): the two green sites of a Bayer quad - Gr beside red, Gb beside blue - see different
crosstalk and differ by a few per cent on many sensor and lens combinations, which the demosaics turn into a one-pixel
checkerboard in flat areas.  Every green pixel moves towards the other green phase by half the difference of the two
phases' local means, where that difference is small enough to be imbalance and both phases are flat enough to be neither
an edge nor texture; every other pixel keeps its bits.

`Camera16/32(green_equalize=GreenEqualize(...))` runs it on every raw frame the loaders take, as the last raw stage,
directly in front of the demosaic; `equalize_cfa` runs it on a normalised CFA on its own.  DESIGN.md 3, "Green
equalisation".
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _native, types
from .bayer import BayerPattern


def _f32_number(name, v, rule, ok):
    """v as a Python float; ValueError unless it is a number that is finite, as a double and in f32, and ok(its f32 value)."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    f = float(v)
    f32 = float(np.float32(f)) if math.isfinite(f) and abs(f) < 3.4e38 else math.inf
    if not math.isfinite(f32) or not ok(f32):
        raise ValueError(f"{name} must be {rule} (in f32 too), got {v!r}")
    return f


@dataclasses.dataclass(frozen=True)
class GreenEqualize:
    """The correction.  With O and S the local means of the other and of the pixel's own green phase (radius 1: 4 and 5
    taps, radius 2: 16 and 9), a green pixel gets x + strength / 2 * (O - S) when |O - S| <= threshold + slope * max(O, S)
    and neither phase's taps span more than edge times that limit; threshold is in the units of the loader's x (1.0 = the
    white level).  The defaults believe an imbalance of up to 1/256 + 6 % of the signal."""
    threshold: float = 1.0 / 256.0
    slope: float = 1.0 / 16.0
    strength: float = 1.0
    radius: int = 1
    edge: float = 4.0

    def __post_init__(self):
        for name in ("threshold", "slope", "edge"):
            _f32_number(f"GreenEqualize.{name}", getattr(self, name), "finite and >= 0", lambda f: f >= 0)
        _f32_number("GreenEqualize.strength", self.strength, "in [0, 1]", lambda f: 0 <= f <= 1)
        if isinstance(self.radius, bool) or not isinstance(self.radius, (int, np.integer)) or self.radius not in (1, 2):
            raise ValueError(f"GreenEqualize.radius must be 1 or 2, got {self.radius!r}")

    def _arg(self) -> "_native.GreenEqualize":
        """The mi_isp_green_equalize of these settings."""
        return _native.GreenEqualize(float(self.threshold), float(self.slope), float(self.strength), int(self.radius),
                                     float(self.edge))


def check_green_equalize(value):
    """The GreenEqualize of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, GreenEqualize):
        return value
    raise ValueError(f"green_equalize must be None or a GreenEqualize, got {type(value).__name__}")


def equalize_cfa(cfa, pattern: BayerPattern, settings: GreenEqualize = GreenEqualize()):
    """The operator on a normalised (H, W) f16 or f32 CFA of any size under the Bayer pattern `pattern` (x = its values, no
    levels, gain or defect map), same dtype out.  numpy in gives numpy out, torch in gives torch out on the same device
    ("Green equalisation")."""
    if not isinstance(settings, GreenEqualize):
        raise ValueError(f"settings must be a GreenEqualize, got {type(settings).__name__}")
    if not isinstance(pattern, BayerPattern):
        raise ValueError(f"pattern must be a BayerPattern, got {type(pattern).__name__}")
    dt = types.ti_type(cfa)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"equalize_cfa takes an f16 or f32 CFA, got {dt}")
    dev = types.to_device(cfa)
    assert dev.ndim == 2, "cfa must be (H, W)"
    H, W = dev.shape
    out = torch.empty_like(dev)
    if H * W:
        _native.check(_native.lib().mi_isp_green_equalize_cfa(dev.data_ptr(), out.data_ptr(), H, W, dt.code, pattern.value,
                                                              settings._arg(), _native.stream_ptr(dev.device)))
    return types.from_device(out, cfa)
