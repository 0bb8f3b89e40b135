"""Output sharpening (an extension): an unsharp mask on the luma of the u8 images the tonemaps return, defined in integer
arithmetic so that its output is the contract's bit for bit ("Output sharpening").

`Camera16/32(sharpen=Sharpen(...))` sharpens every u8 output of the tonemaps and of process_packed12; `unsharp_mask`
filters an (H, W, 3) u8 image on its own, `unsharp_mask_yuv420` the Y plane of a planar YUV 4:2:0 image.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _native, types


def _int_field(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"Sharpen.{name} must be an integer in {lo} .. {hi}, got {v!r}")


@dataclasses.dataclass(frozen=True)
class Sharpen:
    """The output sharpening filter.  amount (0 .. 8) is the gain on the detail, quantised once to 1/64; radius 1 or 2
    takes the 3 x 3 or 5 x 5 binomial blur; threshold (0 .. 255 luma codes) is the soft coring below which detail is left
    alone; overshoot (None, or 0 .. 255) clamps the sharpened luma to the 3 x 3 neighbourhood's range widened by that
    much (the halo clamp)."""
    amount: float = 1.0
    radius: int = 1
    threshold: int = 0
    overshoot: Optional[int] = None

    def __post_init__(self):
        a = self.amount
        if isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)):
            raise ValueError(f"Sharpen.amount must be a number, got {a!r}")
        if not math.isfinite(float(a)) or not 0 <= float(a) <= 8:
            raise ValueError(f"Sharpen.amount must be finite and within [0, 8], got {a!r}")
        if isinstance(self.radius, bool) or not isinstance(self.radius, (int, np.integer)) or self.radius not in (1, 2):
            raise ValueError(f"Sharpen.radius must be 1 or 2, got {self.radius!r}")
        _int_field("threshold", self.threshold, 0, 255)
        if self.overshoot is not None:
            _int_field("overshoot", self.overshoot, 0, 255)

    @property
    def amount_q6(self) -> int:
        """A = floor(amount * 64 + 0.5): the gain the filter multiplies with, 0 .. 512."""
        return int(math.floor(float(self.amount) * 64 + 0.5))

    def _arg(self) -> "_native.Sharpen":
        """The mi_isp_sharpen of these settings."""
        return _native.Sharpen(self.amount_q6, int(self.radius), int(self.threshold),
                               -1 if self.overshoot is None else int(self.overshoot))


def check_sharpen(value):
    """The Sharpen of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, Sharpen):
        return value
    raise ValueError(f"sharpen must be None or a Sharpen, got {type(value).__name__}")


def apply(images, sharpen: Sharpen, yuv420=False):
    """New tensors holding the filter of the u8 device tensors `images` (one shape, contiguous, one device): (H, W, 3)
    images, or with yuv420 planar (H * 3 / 2, W) ones; one launch per 32 images on the device's current stream, no host
    synchronisation."""
    first = images[0]
    outs = [torch.empty_like(im) for im in images]
    if yuv420:
        H, W = first.shape[0] * 2 // 3, first.shape[1]
        fn = _native.lib().mi_isp_sharpen_yuv420_batch
    else:
        H, W = first.shape[:2]
        fn = _native.lib().mi_isp_sharpen_rgb_batch
    if H * W:
        _native.check(fn(_native.ptr_array(images), _native.ptr_array(outs), len(images), H, W, sharpen._arg(),
                         _native.stream_ptr(first.device)))
    return outs


def _checked(image, sharpen, what):
    if not isinstance(sharpen, Sharpen):
        raise ValueError(f"sharpen must be a Sharpen, got {type(sharpen).__name__}")
    if types.ti_type(image) != types.u8:
        raise ValueError(f"{what} takes a u8 image, got {types.ti_type(image)}")
    return types.to_device(image)


def unsharp_mask(image, sharpen: Sharpen):
    """The filter on an (H, W, 3) u8 RGB image: the same delta, computed on the luma, is added to R, G and B, so hue is
    kept up to saturation.  numpy in gives numpy out, torch in gives torch out on the same device (a new tensor: the
    stencil cannot run in place).  DESIGN.md 3, "Output sharpening"."""
    dev = _checked(image, sharpen, "unsharp_mask")
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    return types.from_device(apply([dev], sharpen)[0], image)


def unsharp_mask_yuv420(yuv, sharpen: Sharpen):
    """The filter on a planar YUV 4:2:0 u8 image (H * 3 / 2, W) as color.rgb_yuv420_image makes it: the Y plane (H, W) is
    the luma, out = clamp(Y + delta, 0, 255), and the chroma rows come back unchanged.  This is NOT the YUV image of a
    sharpened RGB image: there the delta comes from the RGB luma (77, 150, 29) / 256 and saturates per channel.
    Containers as unsharp_mask."""
    dev = _checked(yuv, sharpen, "unsharp_mask_yuv420")
    assert dev.ndim == 2 and dev.shape[0] % 3 == 0, "yuv must be (H * 3 / 2, W) with H even"
    return types.from_device(apply([dev], sharpen, yuv420=True)[0], yuv)
