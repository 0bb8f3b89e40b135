"""Bilinear resize and orientation transforms -- call surface of taichi_image/interpolate.py."""
from __future__ import annotations

from enum import Enum

import numpy as np
import torch

from . import _native, types
from .types import as_dtype


class ImageTransform(Enum):
    """interpolate.py:9-17."""
    none = 'none'
    rotate_90 = 'rotate_90'
    rotate_180 = 'rotate_180'
    rotate_270 = 'rotate_270'
    transpose = 'transpose'
    flip_horiz = 'flip_horiz'
    flip_vert = 'flip_vert'
    transverse = 'transverse'


_TRANSFORM_CODE = {t: i for i, t in enumerate(ImageTransform)}


def transform_code(t: ImageTransform) -> int:
    return _TRANSFORM_CODE[t]


def transformed_size(size, transform: ImageTransform):
    """interpolate.py:112-117 (note: `transverse` is not in the swap list in the reference)."""
    w, h = size
    if transform in [ImageTransform.rotate_90, ImageTransform.rotate_270, ImageTransform.transpose]:
        return (h, w)
    return (w, h)


def transform(src, transform: ImageTransform):
    """interpolate.py:119-125.  `transverse` is only defined for square images: the reference
    keeps the source shape for it while its index map needs swapped dims, i.e. it reads out of
    bounds on non-square input; that case raises here instead."""
    dtype = types.ti_type(src)
    dev = types.to_device(src)
    Hs, Ws = dev.shape[:2]
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    assert transform != ImageTransform.transverse or Hs == Ws, "transverse is only defined for square images"
    size = transformed_size((Hs, Ws), transform)
    dst = torch.empty((size[0], size[1], 3), dtype=dtype.torch, device=dev.device)
    _native.check(_native.lib().mi_isp_transform(dev.data_ptr(), dst.data_ptr(), Hs, Ws, dtype.code,
                                                 transform_code(transform), _native.stream_ptr(dev.device)))
    return types.from_device(dst, src)


def _scale2(scale):
    if np.isscalar(scale):
        return float(scale), float(scale)
    s = tuple(float(v) for v in scale)
    assert len(s) == 2, "scale must be a scalar or a (row, col) pair"
    return s


def resize_bilinear(src, size, scale=None, dtype=None):
    """interpolate.py:128-139.  size = (w, h).  scale: scalar or (row_scale, col_scale).
    scale=None reproduces the reference exactly, including its crossed axes
    (vec2(size=(w,h)) / vec2(src.shape=(H,W)), interpolate.py:132-133) -- pass an explicit
    scale for a geometrically correct resize, as camera_isp.ISP always does."""
    in_dtype = types.ti_type(src)
    out_dtype = in_dtype if dtype is None else as_dtype(dtype)
    dev = types.to_device(src)
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    Hs, Ws = dev.shape[:2]
    Wd, Hd = int(size[0]), int(size[1])
    if scale is None:
        scale = (Wd / Hs, Hd / Ws)
    s0, s1 = _scale2(scale)
    dst = torch.empty((Hd, Wd, 3), dtype=out_dtype.torch, device=dev.device)
    _native.check(_native.lib().mi_isp_resize_bilinear(dev.data_ptr(), dst.data_ptr(), Hs, Ws, Hd, Wd, s0, s1,
                                                       in_dtype.code, out_dtype.code,
                                                       _native.stream_ptr(dev.device)))
    return types.from_device(dst, src)


def resample(src, size, scale=None, filter="area", dtype=None):
    """The antialiased resize of an (H, W, 3) f16 or f32 image (an extension; DESIGN.md 3, "Antialiased resize"): the
    separable, table-driven resize of `resample.py` with filter "area", "triangle" or "lanczos3" ("bilinear": exactly
    resize_bilinear at that size and scale).  size = (w, h); scale: a scalar or (row_scale, col_scale), None for
    (h / H, w / W) - geometrically correct, as undistort, not resize_bilinear's crossed axes.  The geometry is
    resize_bilinear's (output index d is centred on source coordinate d / scale), the container rule and the dtype
    handling too; integer images and a scale the filter does not take raise ValueError.  Nothing is clamped."""
    from . import resample as _rs
    _rs.check_filter(filter)
    in_dtype = _rs.float_dtype(src, "resample")
    out_dtype = _rs.out_float_dtype(dtype, in_dtype, "resample")
    assert src.ndim == 3 and src.shape[2] == 3, "image must be (H, W, 3)"
    Hs, Ws = src.shape[:2]
    Wd, Hd = int(size[0]), int(size[1])
    if Wd < 0 or Hd < 0:
        raise ValueError(f"size {tuple(size)} must not be negative")
    if Hs <= 0 or Ws <= 0:
        raise ValueError(f"resample of an empty {Hs} x {Ws} image")
    s0, s1 = (Hd / Hs, Wd / Ws) if scale is None else _scale2(scale)
    if filter == "bilinear":
        return resize_bilinear(src, (Wd, Hd), (s0, s1), dtype)
    _rs.check_geometry(filter, Hs, Ws, Hd, Wd, s0, s1)
    dev = types.to_device(src)
    dst = torch.empty((Hd, Wd, 3), dtype=out_dtype.torch, device=dev.device)
    _rs.apply([dev], [dst], filter, Hs, Ws, Hd, Wd, s0, s1, in_dtype.code, out_dtype.code, dev.device)
    return types.from_device(dst, src)


def resize_width(src, width: int, dtype=None):
    """interpolate.py:141-145 (height truncated with int())."""
    h, w = src.shape[:2]
    scale = width / w
    return resize_bilinear(src, (width, int(h * scale)), scale, dtype)


def scale_bilinear(src, scale, dtype=None):
    """interpolate.py:147-151: size = ivec2(vec2(w, h) * scale) (f32 product, truncated)."""
    h, w = src.shape[:2]
    sw, sh = _scale2(scale)
    size = (int(np.float32(w) * np.float32(sw)), int(np.float32(h) * np.float32(sh)))
    return resize_bilinear(src, size, scale, dtype=dtype)


def undistort(src, lens, size=None, scale=None, dtype=None):
    """Lens distortion correction of an (H, W, 3) image (an extension; DESIGN.md 3, "Lens distortion"): every output pixel
    sampled bilinearly at the source coordinates of `lens` (a lens.LensDistortion of an (H, W) frame), as
    resize_bilinear samples.  size = (w, h) and scale (scalar or (row, col)) of the output as in resize_bilinear: both
    None gives the source size at scale 1; a size alone takes scale (h / H, w / W); a scale alone takes size
    (round(W * s_col), round(H * s_row)).  A table lens gives its table's size and takes no scale.  The container rule and
    the dtype handling are resize_bilinear's."""
    from . import lens as _lens
    in_dtype = types.ti_type(src)
    out_dtype = in_dtype if dtype is None else as_dtype(dtype)
    dev = types.to_device(src)
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    Hs, Ws = dev.shape[:2]
    if not isinstance(lens, _lens.LensDistortion):
        raise ValueError(f"lens must be a LensDistortion, got {type(lens).__name__}")
    if lens.is_table:
        if scale is not None:
            raise ValueError("a lens table gives its own output size: it takes no scale")
        Hd, Wd = lens.table_shape
        if size is not None and (int(size[1]), int(size[0])) != (Hd, Wd):
            raise ValueError(f"size {tuple(size)} is not the lens table's ({Wd}, {Hd})")
        s0 = s1 = 1.0
    elif size is None:
        s0, s1 = (1.0, 1.0) if scale is None else _lens._scale2(scale)
        Hd, Wd = (Hs, Ws) if scale is None else (round(Hs * s0), round(Ws * s1))
    else:
        Wd, Hd = int(size[0]), int(size[1])
        s0, s1 = (Hd / Hs, Wd / Ws) if scale is None else _lens._scale2(scale)
        if Wd < 0 or Hd < 0:
            raise ValueError(f"size {tuple(size)} must not be negative")
    _lens.check_lens(lens, (Hs, Ws), (Hd, Wd))
    dst = torch.empty((Hd, Wd, 3), dtype=out_dtype.torch, device=dev.device)
    if Hd * Wd:
        if not lens.is_table:
            _lens._scale2((s0, s1))
        _lens.apply([lens], [dev], [dst], Hs, Ws, Hd, Wd, s0, s1, in_dtype.code, out_dtype.code, dev.device)
    return types.from_device(dst, src)


def remap(src, map_xy, dtype=None, border="constant"):
    """The table form of undistort: `map_xy` an (Hd, Wd, 2) f32 array of source coordinates (us, vs) (OpenCV's map_x /
    map_y order) for the (H, W, 3) image src; out-of-frame coordinates read 0 (border="constant") or the edge
    ("replicate").  For repeated use keep a lens.LensDistortion.from_map, which caches the table on the device."""
    from . import lens as _lens
    return undistort(src, _lens.LensDistortion.from_map(map_xy, tuple(src.shape[:2]), border), dtype=dtype)
