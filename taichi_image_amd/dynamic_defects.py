"""Dynamic defective-pixel correction (an extension): a raw pixel that stands out of its eight same-site neighbours at
distance 2 by more than a signal-dependent threshold is replaced from the neighbour pair that agrees best - no calibrated
map, no Bayer pattern.  A `DefectMap`, where there is one, stays the authority: its sites are never taps and the static
fix-up replaces them afterwards.

`Camera16/32(dynamic_defects=DynamicDefects(...))` runs it on every raw frame the loaders take, behind exposure merge and
in front of highlight reconstruction; `correct_cfa` runs it on a normalised CFA on its own; `find_defects_dynamic` votes a
`DefectMap` out of ordinary footage.  DESIGN.md 3, "Dynamic defects".
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _native, types
from .defects import DefectMap


def _f32_number(name, v, positive):
    """v as a Python float; ValueError unless it is a number that is finite and > 0 (positive) or >= 0, as a double and
    in f32."""
    rule = "> 0" if positive else ">= 0"
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    f = float(v)
    f32 = float(np.float32(f)) if math.isfinite(f) and abs(f) < 3.4e38 else math.inf
    if not math.isfinite(f32) or not (f32 > 0 if positive else f32 >= 0):
        raise ValueError(f"{name} must be finite and {rule} (in f32 too), got {v!r}")
    return f


@dataclasses.dataclass(frozen=True)
class DynamicDefects:
    """The detector.  A pixel is hot when it exceeds the (tolerate+1)-th largest of its same-site neighbours by more than
    threshold + slope * max(neighbour, 0), dead when it falls below the (tolerate+1)-th smallest by as much; threshold is
    in the units of the loader's x (1.0 = the white level).  tolerate=1 allows one of a pixel's own neighbours to be
    defective itself, so that a same-colour pair of hot pixels is still caught."""
    threshold: float = 0.02
    slope: float = 0.2
    tolerate: int = 1
    hot: bool = True
    dead: bool = True

    def __post_init__(self):
        _f32_number("DynamicDefects.threshold", self.threshold, positive=True)
        _f32_number("DynamicDefects.slope", self.slope, positive=False)
        if isinstance(self.tolerate, bool) or not isinstance(self.tolerate, (int, np.integer)) or self.tolerate not in (0, 1):
            raise ValueError(f"DynamicDefects.tolerate must be 0 or 1, got {self.tolerate!r}")
        for name in ("hot", "dead"):
            if not isinstance(getattr(self, name), (bool, np.bool_)):
                raise ValueError(f"DynamicDefects.{name} must be a bool, got {getattr(self, name)!r}")
        if not (self.hot or self.dead):
            raise ValueError("DynamicDefects: at least one of hot and dead must be True")

    def _arg(self) -> "_native.DynamicDefects":
        """The mi_isp_dynamic_defects of these settings."""
        return _native.DynamicDefects(float(self.threshold), float(self.slope), int(self.tolerate), int(bool(self.hot)),
                                      int(bool(self.dead)))


def check_dynamic_defects(value):
    """The DynamicDefects of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, DynamicDefects):
        return value
    raise ValueError(f"dynamic_defects must be None or a DynamicDefects, got {type(value).__name__}")


def _unpack_flags(words: torch.Tensor, W: int) -> torch.Tensor:
    """The 0 / 1 int32 (..., H, W) plane of (..., H, ceil(W / 32)) int32 flag words in DefectMap.mask_words() layout."""
    bit = torch.arange(32, dtype=torch.int32, device=words.device)
    bits = (words.unsqueeze(-1) >> bit) & 1                 # (an arithmetic shift: the sign bit is masked off again)
    return bits.reshape(*words.shape[:-1], words.shape[-1] * 32)[..., :W]


def _vote(words: torch.Tensor, W: int, min_hits: int) -> torch.Tensor:
    """The boolean (H, W) mask of the sites set in at least min_hits of the K planes of (K, H, ceil(W / 32)) flag words."""
    return _unpack_flags(words, W).sum(dim=0) >= min_hits


def _run(dev, settings, mask_arg, want_flags):
    """(the corrected CFA, the int32 flag words or None) of the (H, W) f16 / f32 device tensor dev."""
    H, W = dev.shape
    dt = types.ti_type(dev)
    out = torch.empty_like(dev)
    words = torch.empty((H, (W + 31) // 32), dtype=torch.int32, device=dev.device) if want_flags else None
    if H * W:
        L = _native.lib()
        stream = _native.stream_ptr(dev.device)
        if mask_arg is None:
            _native.check(L.mi_isp_dynamic_defects_cfa(dev.data_ptr(), out.data_ptr(), H, W, dt.code, settings._arg(), stream,
                                                       None if words is None else words.data_ptr()))
        else:       # a normalised CFA with a map: the f32 source kind, or f16 widened (exact) to it
            src = dev if dev.dtype == torch.float32 else dev.float()
            _native.check(L.mi_isp_dynamic_defects_raw(src.data_ptr(), out.data_ptr(), H, W, _native.MI_RAW_32F, 0, dt.code,
                                                       None, None, mask_arg, settings._arg(), 0, stream,
                                                       None if words is None else words.data_ptr()))
    return out, words


def correct_cfa(cfa, settings: DynamicDefects = DynamicDefects(), defects=None, return_flags=False):
    """The operator on a normalised (H, W) f16 or f32 CFA of any size (x = its values, no levels or gain), same dtype out.
    defects: the DefectMap of the frame (its sites are never taps and keep their value) or None.  With return_flags the
    result is (cfa, the boolean (H, W) mask of the pixels that were hot or dead).  numpy in gives numpy out, torch in gives
    torch out on the same device ("Dynamic defects")."""
    if not isinstance(settings, DynamicDefects):
        raise ValueError(f"settings must be a DynamicDefects, got {type(settings).__name__}")
    if defects is not None and not isinstance(defects, DefectMap):
        raise ValueError(f"defects must be None or a DefectMap, got {type(defects).__name__}")
    dt = types.ti_type(cfa)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"correct_cfa takes an f16 or f32 CFA, got {dt}")
    if defects is not None and tuple(defects.shape) != tuple(cfa.shape):
        raise ValueError(f"the DefectMap is of a {defects.shape} frame, the CFA is {tuple(cfa.shape)}")
    dev = types.to_device(cfa)
    assert dev.ndim == 2, "cfa must be (H, W)"
    H, W = dev.shape
    arg = None if defects is None else defects._arg(dev.device)
    out, words = _run(dev, settings, arg, bool(return_flags))
    res = types.from_device(out, cfa)
    if not return_flags:
        return res
    return res, types.from_device(_unpack_flags(words, W).bool(), cfa)


def find_defects_dynamic(frames, settings: DynamicDefects, min_hits: int) -> DefectMap:
    """The DefectMap of the sites the detector flags in at least min_hits of the K frames of a (K, H, W) stack of
    normalised f16 or f32 CFAs (H and W even): find_defects for ordinary footage instead of dark and flat frames.  A
    persistent defect is flagged in almost every frame, scene detail in few."""
    if not isinstance(settings, DynamicDefects):
        raise ValueError(f"settings must be a DynamicDefects, got {type(settings).__name__}")
    dt = types.ti_type(frames)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"find_defects_dynamic takes f16 or f32 frames, got {dt}")
    if frames.ndim != 3 or frames.shape[0] < 1:
        raise ValueError(f"frames must be (K, H, W), got shape {tuple(frames.shape)}")
    K, H, W = (int(v) for v in frames.shape)
    if isinstance(min_hits, bool) or not isinstance(min_hits, (int, np.integer)) or not 1 <= min_hits <= K:
        raise ValueError(f"min_hits must be an integer in 1 .. {K}, got {min_hits!r}")
    dev = types.to_device(frames)
    words = torch.stack([_run(dev[k].contiguous(), settings, None, True)[1] for k in range(K)])
    return DefectMap.from_mask(_vote(words, W, int(min_hits)))
