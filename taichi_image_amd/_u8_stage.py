"""What the filters on the u8 outputs share on the Python side (sharpen, local_contrast, chroma_denoise, luma_denoise,
color_lut): the validators of their settings' fields, the 1/64 quantiser, the check of a constructor / set() argument, the
geometry of the RGB and the planar YUV 4:2:0 form, and the call of a batch entry point.  The messages name the settings class,
so each module's texts are its own."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native, types


def int_field(cls, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{cls}.{name} must be an integer in {lo} .. {hi}, got {v!r}")


def number(cls, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{cls}.{name} must be a number, got {v!r}")
    if not math.isfinite(float(v)) or not lo <= float(v) <= hi:
        raise ValueError(f"{cls}.{name} must be finite and within [{lo}, {hi}], got {v!r}")


def q6(x) -> int:
    """floor(x * 64 + 0.5): a strength or an amount as the kernels multiply with it."""
    return int(math.floor(float(x) * 64 + 0.5))


def check_setting(value, cls, name):
    """The `cls` of a constructor / set() argument `name`, None for None; ValueError otherwise."""
    if value is None or isinstance(value, cls):
        return value
    raise ValueError(f"{name} must be None or a {cls.__name__}, got {type(value).__name__}")


def geometry(image, yuv420):
    """(H, W) of an (H, W, 3) image, or with yuv420 of the Y plane of a planar (H * 3 / 2, W) one."""
    return (image.shape[0] * 2 // 3, image.shape[1]) if yuv420 else tuple(image.shape[:2])


def apply_batch(images, fn_rgb, fn_yuv, arg, yuv420=False, inplace=False, extra=()):
    """The batch entry point fn_rgb (fn_yuv with yuv420; names of the library) on the u8 device tensors `images` (one shape,
    contiguous, one device): `arg`, then `extra`, are the arguments between the shape and the stream.
    inplace=True overwrites and returns `images`, else new tensors come back.  On the device's current stream, no host
    synchronisation; an empty image launches nothing."""
    first = images[0]
    H, W = geometry(first, yuv420)
    outs = images if inplace else [torch.empty_like(im) for im in images]
    if H * W:
        fn = getattr(_native.lib(), fn_yuv if yuv420 else fn_rgb)
        _native.check(fn(_native.ptr_array(images), _native.ptr_array(outs), len(images), H, W, arg, *extra,
                         _native.stream_ptr(first.device)))
    return outs


def checked(image, settings, cls, what, name="settings"):
    """The device tensor of a public function's u8 `image`; ValueError for other settings than a `cls` or another dtype."""
    if not isinstance(settings, cls):
        raise ValueError(f"{name} must be a {cls.__name__}, got {type(settings).__name__}")
    if types.ti_type(image) != types.u8:
        raise ValueError(f"{what} takes a u8 image, got {types.ti_type(image)}")
    return types.to_device(image)
