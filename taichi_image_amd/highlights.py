"""Highlight reconstruction (an extension): raw pixels at the sensor's clip level are rebuilt from the white-balanced
values of their neighbours, so a blown-out region comes out neutral instead of magenta.

`Camera16/32(highlights=Highlights(...))` runs it on every raw frame the loaders take, after levels and before raw noise
reduction, shading and the cast; `reconstruct_cfa` runs it on a normalised CFA on its own.  DESIGN.md 3, "Highlight
reconstruction".
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _native, bayer, types

MODES = ("rebuild", "clip")


def _positive_f32(name, v):
    """v as a Python float; ValueError unless it is a number that is finite and > 0, as a double and in f32."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    f = float(v)
    f32 = float(np.float32(f)) if math.isfinite(f) and abs(f) < 3.4e38 else math.inf
    if not math.isfinite(f32) or not f32 > 0:
        raise ValueError(f"{name} must be finite and > 0 (in f32 too), got {v!r}")
    return f


@dataclasses.dataclass(frozen=True)
class Highlights:
    """The highlight operator.  mode "rebuild" raises a pixel with x >= clip to the brightest balanced mean of its
    neighbour colours (only clipped pixels change, none is lowered); mode "clip" limits every pixel to the balanced clip
    level clip * min(w) / w[site].  clip is in the units of the loader's x (1.0 = the white level)."""
    mode: str = "rebuild"
    clip: float = 0.98

    def __post_init__(self):
        if not isinstance(self.mode, str) or self.mode not in MODES:
            raise ValueError(f"Highlights.mode must be one of {MODES}, got {self.mode!r}")
        _positive_f32("Highlights.clip", self.clip)

    def _arg(self, white_balance=(1.0, 1.0, 1.0), gains_dev=None) -> "_native.Highlights":
        """The mi_isp_highlights of these settings with the balance gains white_balance (R, G, B), or with the 3 f32 of
        the device tensor gains_dev, which the kernel reads."""
        wb = [float(np.float32(v)) for v in white_balance]
        return _native.Highlights(MODES.index(self.mode), float(self.clip), (_native.c_float * 3)(*wb),
                                  None if gains_dev is None else gains_dev.data_ptr())


def check_highlights(value):
    """The Highlights of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, Highlights):
        return value
    raise ValueError(f"highlights must be None or a Highlights, got {type(value).__name__}")


def check_white_balance(white_balance):
    """(w_R, w_G, w_B) as f32 values: three numbers, finite and > 0 in f32; ValueError otherwise."""
    try:
        wb = [v for v in white_balance]
    except TypeError:
        raise ValueError(f"white_balance must be three numbers, got {white_balance!r}") from None
    if len(wb) != 3:
        raise ValueError(f"white_balance must be three numbers (R, G, B), got {len(wb)}")
    return tuple(float(np.float32(_positive_f32("white_balance", v))) for v in wb)


def reconstruct_cfa(cfa, pattern, white_balance=(1.0, 1.0, 1.0), highlights: Highlights = Highlights()):
    """The operator on a normalised (H, W) f16 or f32 CFA of Bayer pattern `pattern` (x = its values, no levels, gain or
    defects), same dtype out.  numpy in gives numpy out, torch in gives torch out on the same device (DESIGN.md 3,
    "Highlight reconstruction")."""
    if not isinstance(highlights, Highlights):
        raise ValueError(f"highlights must be a Highlights, got {type(highlights).__name__}")
    if not isinstance(pattern, bayer.BayerPattern):
        raise ValueError(f"pattern must be a BayerPattern, got {type(pattern).__name__}")
    wb = check_white_balance(white_balance)
    dt = types.ti_type(cfa)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"reconstruct_cfa takes an f16 or f32 CFA, got {dt}")
    dev = types.to_device(cfa)
    assert dev.ndim == 2, "cfa must be (H, W)"
    H, W = dev.shape
    out = torch.empty_like(dev)
    if H * W:
        _native.check(_native.lib().mi_isp_highlights_cfa(dev.data_ptr(), out.data_ptr(), H, W, dt.code, pattern.value,
                                                          highlights._arg(wb), _native.stream_ptr(dev.device)))
    return types.from_device(out, cfa)
