"""Lateral chromatic aberration correction (an extension): the red and blue site planes of the CFA are resampled radially
about the optical centre, so that they register with green before the demosaic turns a misregistration into false colour.

`Camera16/32(chromatic_aberration=ChromaticAberration(...))` runs it on every raw frame the loaders take, after levels and
highlight reconstruction and before raw noise reduction, shading and the cast; `correct_cfa` runs it on a normalised CFA on
its own.  DESIGN.md 3, "Chromatic aberration".
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native, bayer, types

MAX_SHIFT = 8.0            # raw pixels: the largest shift the kernel's halo covers
SHIFT_SAMPLES = 1025       # radii at which max_shift evaluates the shift


def _finite_f32(name, v):
    """v as a Python float; ValueError unless it is a number that is finite, as a double and in f32."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    f = float(v)
    if not math.isfinite(f) or abs(f) > 3.4e38:
        raise ValueError(f"{name} must be finite (in f32 too), got {v!r}")
    return f


def _numbers(name, value, n):
    try:
        vs = tuple(value)
    except TypeError:
        raise ValueError(f"{name} must be {n} numbers, got {value!r}") from None
    if len(vs) != n:
        raise ValueError(f"{name} must be {n} numbers, got {len(vs)}")
    return tuple(_finite_f32(name, v) for v in vs)


@functools.lru_cache(maxsize=64)
def _max_shift(k, cy, cx, nr, H, W):
    """The largest |(k0 - 1) + q (k1 + q k2)| r of a channel on an H x W frame (ChromaticAberration.max_shift; cached: the
    loaders ask at every call)."""
    ry = max(abs(cy), abs((H - 1) - cy))
    rx = max(abs(cx), abs((W - 1) - cx))
    rmax = math.sqrt(ry * ry + rx * rx)
    n2 = nr * nr
    worst = 0.0
    for i in range(SHIFT_SAMPLES):
        r = rmax * float(i) / float(SHIFT_SAMPLES - 1)
        q = r * r / n2
        shift = abs((k[0] - 1.0) + q * (k[1] + q * k[2])) * r
        if not shift <= worst:
            worst = shift
    return worst


@dataclasses.dataclass(frozen=True)
class ChromaticAberration:
    """The lens' lateral colour.  red, blue: (k0, k1, k2) of the channel's scale s(q) = k0 + k1 q + k2 q^2 at normalised
    squared radius q = r^2 / norm_radius^2: the output pixel at p takes its channel from centre + s (p - centre).  center:
    (cy, cx) in raw pixels, None for the middle of the frame ((H - 1) / 2, (W - 1) / 2); norm_radius in raw pixels, None
    for hypot(H / 2, W / 2).  The shift |s - 1| r may not exceed 8 raw pixels anywhere on a frame (ValueError at the load)."""
    red: Tuple[float, float, float] = (1.0, 0.0, 0.0)
    blue: Tuple[float, float, float] = (1.0, 0.0, 0.0)
    center: Optional[Tuple[float, float]] = None
    norm_radius: Optional[float] = None

    def __post_init__(self):
        object.__setattr__(self, "red", _numbers("ChromaticAberration.red", self.red, 3))
        object.__setattr__(self, "blue", _numbers("ChromaticAberration.blue", self.blue, 3))
        if self.center is not None:
            object.__setattr__(self, "center", _numbers("ChromaticAberration.center", self.center, 2))
        if self.norm_radius is not None:
            r = _finite_f32("ChromaticAberration.norm_radius", self.norm_radius)
            if not r > 0 or not math.isfinite(1.0 / (r * r)) or 1.0 / (r * r) > 3.4e38:
                raise ValueError(f"ChromaticAberration.norm_radius must be > 0 (1 / r^2 finite in f32), got {self.norm_radius!r}")
            object.__setattr__(self, "norm_radius", r)

    def _geometry(self, shape):
        """(cy, cx, norm_radius) on a frame of `shape` = (H, W), as doubles."""
        H, W = int(shape[0]), int(shape[1])
        cy, cx = ((H - 1) / 2.0, (W - 1) / 2.0) if self.center is None else self.center
        return cy, cx, (math.hypot(H / 2.0, W / 2.0) if self.norm_radius is None else self.norm_radius)

    def max_shift(self, shape):
        """(red, blue): the largest |(k0 - 1) + q (k1 + q k2)| r of each channel on a frame of `shape`, in double, at 1025
        equally spaced radii r from 0 to the distance of the farthest corner pixel from the centre."""
        H, W = int(shape[0]), int(shape[1])
        cy, cx, nr = self._geometry(shape)
        return _max_shift(self.red, cy, cx, nr, H, W), _max_shift(self.blue, cy, cx, nr, H, W)

    def check_shape(self, shape):
        """ValueError when the shift on a frame of `shape` exceeds the limit (before anything is uploaded or launched)."""
        H, W = int(shape[0]), int(shape[1])
        if H * W == 0:
            return
        if self.norm_radius is None and not math.hypot(H / 2.0, W / 2.0) > 0:
            raise ValueError(f"chromatic aberration: no norm_radius for a {H}x{W} frame")
        red, blue = self.max_shift(shape)
        if not (red <= MAX_SHIFT and blue <= MAX_SHIFT):
            raise ValueError(f"chromatic aberration shift (red {red:.6g}, blue {blue:.6g} raw pixels on a {H}x{W} frame) "
                             f"exceeds {MAX_SHIFT:g}")

    def _arg(self, shape) -> "_native.Chromatic":
        """The mi_isp_chromatic of these settings on a frame of `shape` (the defaults of center and norm_radius resolved)."""
        cy, cx, nr = self._geometry(shape)
        return _native.Chromatic(cy, cx, nr, (_native.c_double * 3)(*self.red), (_native.c_double * 3)(*self.blue))


def check_chromatic_aberration(value):
    """The ChromaticAberration of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, ChromaticAberration):
        return value
    raise ValueError(f"chromatic_aberration must be None or a ChromaticAberration, got {type(value).__name__}")


def correct_cfa(cfa, pattern, ca: ChromaticAberration):
    """The operator on a normalised (H, W) f16 or f32 CFA of Bayer pattern `pattern` (x = its values, no levels, gain or
    defects), same dtype out.  numpy in gives numpy out, torch in gives torch out on the same device (DESIGN.md 3,
    "Chromatic aberration")."""
    if not isinstance(ca, ChromaticAberration):
        raise ValueError(f"ca must be a ChromaticAberration, got {type(ca).__name__}")
    if not isinstance(pattern, bayer.BayerPattern):
        raise ValueError(f"pattern must be a BayerPattern, got {type(pattern).__name__}")
    dt = types.ti_type(cfa)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"correct_cfa takes an f16 or f32 CFA, got {dt}")
    if cfa.ndim != 2:
        raise ValueError("cfa must be (H, W)")
    ca.check_shape(cfa.shape)
    dev = types.to_device(cfa)
    H, W = dev.shape
    out = torch.empty_like(dev)
    if H * W:
        _native.check(_native.lib().mi_isp_chromatic_cfa(dev.data_ptr(), out.data_ptr(), H, W, dt.code, pattern.value,
                                                         ca._arg((H, W)), _native.stream_ptr(dev.device)))
    return types.from_device(out, cfa)
