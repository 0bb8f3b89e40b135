"""Antialiased resize (an extension): a separable, table-driven resize with an area (box), a triangle or a Lanczos-3
filter that widens with the downscale, where `interpolate.resize_bilinear` reads a 2 x 2 neighbourhood whatever the scale
and so aliases below scale 1.

`Camera16/32(resample=Resample("area"))` resizes every loader's images with it; `interpolate.resample` runs it on an image
on its own.  DESIGN.md 3, "Antialiased resize".
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

from . import _native, types
from .types import as_dtype

FILTERS = ("bilinear", "area", "triangle", "lanczos3")
MAX_TAPS = 32
# MI_RESAMPLE_*
_FILTER_CODE = {"area": 1, "triangle": 2, "lanczos3": 3}


@dataclasses.dataclass(frozen=True)
class Resample:
    """The resize of an ISP.  filter "area": the mean over the source pixels an output pixel covers; "triangle": a tent
    as wide as two output pixels; "lanczos3": the windowed sinc (sharpest; it can overshoot and go negative); "bilinear":
    the point-sampled resize, as without the option.  Every filter takes scales down to the one at which an axis needs
    more than 32 taps: 1 / 31 (area), 1 / 16 (triangle), 3 / 16 (lanczos3)."""
    filter: str = "area"

    def __post_init__(self):
        check_filter(self.filter, "Resample.filter")

    @property
    def is_bilinear(self) -> bool:
        return self.filter == "bilinear"


def check_filter(name, what="filter"):
    if not isinstance(name, str) or name not in FILTERS:
        raise ValueError(f"{what} must be one of {FILTERS}, got {name!r}")
    return name


def check_resample(value):
    """The Resample of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, Resample):
        return value
    raise ValueError(f"resample must be None or a Resample, got {type(value).__name__}")


def _axis_args(filter, S, D, scale):
    check_filter(filter)
    if filter == "bilinear":
        raise ValueError("the bilinear resize has no table: it is interpolate.resize_bilinear")
    for what, v in (("source", S), ("output", D)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
            raise ValueError(f"resample: the {what} samples of an axis must be a positive int, got {v!r}")
    scale = float(scale)
    return _FILTER_CODE[filter], int(S), int(D), scale


def taps(filter, S, D, scale) -> int:
    """T of the axis of S source and D output samples at `scale` (output / source) under `filter`; ValueError when the
    filter does not take the scale (T > 32: the text names the filter and its smallest scale) or for bad arguments."""
    args = _axis_args(filter, S, D, scale)
    T = _native.lib().mi_isp_resample_taps(*args)
    if T < 0:
        raise ValueError("libmi355_isp: " + _native.lib().mi_isp_last_error().decode("utf-8", "replace"))
    return int(T)


def table(filter, S, D, scale):
    """The table of an axis as the kernel takes it, built by the library on the host: (T, start int32[D], weight
    f32[D, T]).  DESIGN.md 3, "Antialiased resize"."""
    args = _axis_args(filter, S, D, scale)
    T = taps(filter, S, D, scale)
    start = np.empty(args[2], dtype=np.int32)
    weight = np.empty((args[2], T), dtype=np.float32)
    if _native.lib().mi_isp_resample_table(*args, start.ctypes.data, weight.ctypes.data):
        raise ValueError("libmi355_isp: " + _native.lib().mi_isp_last_error().decode("utf-8", "replace"))
    return T, start, weight


_tables: dict = {}


def _device_axis(filter, S, D, scale, device):
    """The uploaded table of an axis on `device`: (ResampleAxis, the tensors that back it), built and copied once per
    (device, filter, S, D, scale) and kept for the life of the process, so a later call of the geometry copies nothing and
    can be captured into a graph."""
    key = (device.type, device.index or 0, filter, int(S), int(D), float(scale))
    hit = _tables.get(key)
    if hit is None:
        T, start, weight = table(filter, S, D, scale)
        start_dev, weight_dev = torch.from_numpy(start).to(device), torch.from_numpy(weight).to(device)
        hit = (_native.ResampleAxis(T, start_dev.data_ptr(), weight_dev.data_ptr()), start_dev, weight_dev)
        _tables[key] = hit
    return hit


def check_geometry(filter, Hs, Ws, Hd, Wd, s0, s1):
    """ValueError when `filter` does not take the (row, col) scales (s0, s1) of an Hs x Ws -> Hd x Wd resize; nothing
    is uploaded or launched."""
    if Hd > 0 and Wd > 0:
        taps(filter, Hs, Hd, s0)
        taps(filter, Ws, Wd, s1)


def apply(srcs, dsts, filter, Hs, Ws, Hd, Wd, s0, s1, in_code, out_code, device):
    """The (Hs, Ws, 3) device images srcs resampled into the (Hd, Wd, 3) images dsts at the (row, col) scales (s0, s1):
    ONE launch for all of them (per 32)."""
    if not srcs or Hd * Wd == 0:
        return
    rows = _device_axis(filter, Hs, Hd, s0, device)
    cols = _device_axis(filter, Ws, Wd, s1, device)
    _native.check(_native.lib().mi_isp_resample_batch(
        _native.ptr_array(srcs), _native.ptr_array(dsts), len(srcs), Hs, Ws, Hd, Wd, in_code, out_code,
        ctypes.byref(rows[0]), ctypes.byref(cols[0]), _native.stream_ptr(device)))


def float_dtype(image, what="resample"):
    """The library dtype of a float image; ValueError for an integer one (or one the library has no name for)."""
    try:
        dt = types.ti_type(image)
    except KeyError:
        dt = getattr(image, "dtype", None)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"{what} takes f16 or f32 images, got {dt}")
    return dt


def out_float_dtype(dtype, in_dtype, what="resample"):
    out = in_dtype if dtype is None else as_dtype(dtype)
    if out not in (types.f16, types.f32):
        raise ValueError(f"{what} writes f16 or f32 images, got {out}")
    return out
