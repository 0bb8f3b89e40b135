"""Luma noise reduction (an extension): an edge-preserving mean of the luma over a (2r + 1)^2 window of the u8 images the
tonemaps return, defined in integer arithmetic so that its output is the contract's bit for bit ("Luma noise
reduction").

`Camera16/32(luma_denoise=LumaDenoise(...))` filters every u8 output of the tonemaps and of process_packed12, behind chroma
noise reduction and before local contrast and sharpening; `luma_denoise` filters an (H, W, 3) u8 image on its own,
`luma_denoise_yuv420` the Y plane of a planar YUV 4:2:0 image.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

from . import _native, _u8_stage as _u8, types


@dataclasses.dataclass(frozen=True)
class LumaDenoise:
    """The luma noise filter.  radius (1, 2 or 3) is the window in pixels: 9, 25 or 49 taps; a tap counts when its luma is
    within the pixel's threshold of the pixel's own, and the threshold moves with the pixel's luma from `threshold` (0 ..
    255 luma codes) in the dark to `threshold_bright` in the bright (None: the same as `threshold`); strength (0 .. 1) is
    how far the luma moves to the mean of those taps, quantised once to 1/64."""
    radius: int = 2
    threshold: int = 6
    threshold_bright: Optional[int] = None
    strength: float = 1.0

    def __post_init__(self):
        _u8.int_field("LumaDenoise", "radius", self.radius, 1, 3)
        _u8.int_field("LumaDenoise", "threshold", self.threshold, 0, 255)
        if self.threshold_bright is not None:
            _u8.int_field("LumaDenoise", "threshold_bright", self.threshold_bright, 0, 255)
        _u8.number("LumaDenoise", "strength", self.strength, 0, 1)

    @property
    def strength_q6(self) -> int:
        """S = floor(strength * 64 + 0.5): the weight the filter multiplies with, 0 .. 64."""
        return _u8.q6(self.strength)

    def _arg(self) -> "_native.LumaDenoise":
        """The mi_isp_luma_denoise of these settings."""
        bright = self.threshold if self.threshold_bright is None else self.threshold_bright
        return _native.LumaDenoise(int(self.radius), int(self.threshold), int(bright), self.strength_q6)


def check_luma_denoise(value):
    """The LumaDenoise of a constructor / set() argument, None for None; ValueError otherwise."""
    return _u8.check_setting(value, LumaDenoise, "luma_denoise")


def apply(images, settings: LumaDenoise, yuv420=False):
    """New tensors holding the filter of the u8 device tensors `images` (one shape, contiguous, one device): (H, W, 3)
    images, or with yuv420 planar (H * 3 / 2, W) ones; one launch per 32 images (and one copy of the chroma rows for the
    planar form) on the device's current stream, no host synchronisation."""
    return _u8.apply_batch(images, "mi_isp_luma_denoise_rgb_batch", "mi_isp_luma_denoise_yuv420_batch", settings._arg(),
                           yuv420)


def luma_denoise(image, settings: LumaDenoise):
    """The filter on an (H, W, 3) u8 RGB image: the luma of each pixel moves toward the mean of the window's similar lumas,
    and R, G and B take the same delta, so hue and saturation stay up to the clip.  numpy in gives numpy out, torch in
    gives torch out on the same device (a new tensor: the stencil cannot run in place).  DESIGN.md 3, "Luma noise
    reduction"."""
    dev = _u8.checked(image, settings, LumaDenoise, "luma_denoise")
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    return types.from_device(apply([dev], settings)[0], image)


def luma_denoise_yuv420(yuv, settings: LumaDenoise):
    """The filter on a planar YUV 4:2:0 u8 image (H * 3 / 2, W; H and W even) as color.split_yuv_420 reads it: the Y plane
    filtered with L = Y, the chroma rows unchanged.  Containers as luma_denoise."""
    dev = _u8.checked(yuv, settings, LumaDenoise, "luma_denoise_yuv420")
    assert dev.ndim == 2 and dev.shape[0] % 3 == 0 and dev.shape[1] % 2 == 0, "yuv must be (H * 3 / 2, W) with H, W even"
    return types.from_device(apply([dev], settings, yuv420=True)[0], yuv)
