"""Output sharpening (an extension): an unsharp mask on the luma of the u8 images the tonemaps return, defined in integer
arithmetic so that its output is the contract's bit for bit ("Output sharpening").

`Camera16/32(sharpen=Sharpen(...))` sharpens every u8 output of the tonemaps and of process_packed12; `unsharp_mask`
filters an (H, W, 3) u8 image on its own, `unsharp_mask_yuv420` the Y plane of a planar YUV 4:2:0 image.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

from . import _native, _u8_stage as _u8, types


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
        _u8.number("Sharpen", "amount", self.amount, 0, 8)
        if isinstance(self.radius, bool) or not isinstance(self.radius, (int, np.integer)) or self.radius not in (1, 2):
            raise ValueError(f"Sharpen.radius must be 1 or 2, got {self.radius!r}")
        _u8.int_field("Sharpen", "threshold", self.threshold, 0, 255)
        if self.overshoot is not None:
            _u8.int_field("Sharpen", "overshoot", self.overshoot, 0, 255)

    @property
    def amount_q6(self) -> int:
        """A = floor(amount * 64 + 0.5): the gain the filter multiplies with, 0 .. 512."""
        return _u8.q6(self.amount)

    def _arg(self) -> "_native.Sharpen":
        """The mi_isp_sharpen of these settings."""
        return _native.Sharpen(self.amount_q6, int(self.radius), int(self.threshold),
                               -1 if self.overshoot is None else int(self.overshoot))


def check_sharpen(value):
    """The Sharpen of a constructor / set() argument, None for None; ValueError otherwise."""
    return _u8.check_setting(value, Sharpen, "sharpen")


def apply(images, sharpen: Sharpen, yuv420=False):
    """New tensors holding the filter of the u8 device tensors `images` (one shape, contiguous, one device): (H, W, 3)
    images, or with yuv420 planar (H * 3 / 2, W) ones; one launch per 32 images on the device's current stream, no host
    synchronisation."""
    return _u8.apply_batch(images, "mi_isp_sharpen_rgb_batch", "mi_isp_sharpen_yuv420_batch", sharpen._arg(), yuv420)


def unsharp_mask(image, sharpen: Sharpen):
    """The filter on an (H, W, 3) u8 RGB image: the same delta, computed on the luma, is added to R, G and B, so hue is
    kept up to saturation.  numpy in gives numpy out, torch in gives torch out on the same device (a new tensor: the
    stencil cannot run in place).  DESIGN.md 3, "Output sharpening"."""
    dev = _u8.checked(image, sharpen, Sharpen, "unsharp_mask", "sharpen")
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    return types.from_device(apply([dev], sharpen)[0], image)


def unsharp_mask_yuv420(yuv, sharpen: Sharpen):
    """The filter on a planar YUV 4:2:0 u8 image (H * 3 / 2, W) as color.rgb_yuv420_image makes it: the Y plane (H, W) is
    the luma, out = clamp(Y + delta, 0, 255), and the chroma rows come back unchanged.  This is NOT the YUV image of a
    sharpened RGB image: there the delta comes from the RGB luma (77, 150, 29) / 256 and saturates per channel.
    Containers as unsharp_mask."""
    dev = _u8.checked(yuv, sharpen, Sharpen, "unsharp_mask_yuv420", "sharpen")
    assert dev.ndim == 2 and dev.shape[0] % 3 == 0, "yuv must be (H * 3 / 2, W) with H even"
    return types.from_device(apply([dev], sharpen, yuv420=True)[0], yuv)
