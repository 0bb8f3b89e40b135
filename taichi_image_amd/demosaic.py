"""Direction-adaptive demosaic (an extension): an alternative to the 13-tap filter of `bayer.bayer_to_rgb` that
interpolates green along the direction in which the colour differences vary least, so fine stripes and edges come out
without the zipper and false colour a linear filter leaves on them.

`Camera16/32(demosaic=Demosaic("directional"))` demosaics every frame the loaders take with it; `directional` runs it on a
normalised CFA on its own.  DESIGN.md 3, "Directional demosaic".
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np
import torch

from . import _native, bayer, types
from .types import as_dtype

METHODS = ("malvar", "directional")


@dataclasses.dataclass(frozen=True)
class Demosaic:
    """The demosaic of an ISP.  method "directional": the direction-adaptive operator; "malvar": the 13-tap filter, as
    without the option."""
    method: str = "directional"

    def __post_init__(self):
        if not isinstance(self.method, str) or self.method not in METHODS:
            raise ValueError(f"Demosaic.method must be one of {METHODS}, got {self.method!r}")

    @property
    def is_directional(self) -> bool:
        return self.method == "directional"


def check_demosaic(value):
    """The Demosaic of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, Demosaic):
        return value
    raise ValueError(f"demosaic must be None or a Demosaic, got {type(value).__name__}")


def directional(cfa, pattern: bayer.BayerPattern = bayer.BayerPattern.RGGB, correct_colors: Optional[np.ndarray] = None,
                dtype=None):
    """The operator on a normalised (H, W) f16 or f32 CFA, H and W even: the (H, W, 3) image of `dtype` (None: the
    CFA's), through `bayer_to_rgb`'s epilogue (the optional 3x3 matrix, the clamp to [0, 1], the output's scale and
    cast).  numpy in gives numpy out, torch in gives torch out on the same device."""
    if not isinstance(pattern, bayer.BayerPattern):
        raise ValueError(f"pattern must be a BayerPattern, got {type(pattern).__name__}")
    try:
        in_dtype = types.ti_type(cfa)
    except KeyError:                             # (a dtype the library has no name for)
        in_dtype = getattr(cfa, "dtype", None)
    if in_dtype not in (types.f16, types.f32):
        raise ValueError(f"directional takes an f16 or f32 CFA, got {in_dtype}")
    assert cfa.ndim == 2, "image must be mono bayer"
    assert cfa.shape[0] % 2 == 0 and cfa.shape[1] % 2 == 0, "image must be even size"
    out_dtype = in_dtype if dtype is None else as_dtype(dtype)
    dev = types.to_device(cfa)
    H, W = dev.shape
    rgb = torch.empty((H, W, 3), dtype=out_dtype.torch, device=dev.device)
    if H * W:
        _native.check(_native.lib().mi_isp_demosaic_directional_cfa(
            dev.data_ptr(), rgb.data_ptr(), H, W, in_dtype.code, out_dtype.code, pattern.value,
            _native.ccm_arg(correct_colors), _native.stream_ptr(dev.device)))
    return types.from_device(rgb, cfa)
