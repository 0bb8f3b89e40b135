"""Chroma noise reduction (an extension): a luma-guided mean of the chroma on the grid of 2 x 2 pixel cells of the u8 images
the tonemaps return, defined in integer arithmetic so that its output is the contract's bit for bit ("Chroma
noise reduction").

`Camera16/32(chroma_denoise=ChromaDenoise(...))` filters every u8 output of the tonemaps and of process_packed12, before
local contrast and sharpening; `chroma_denoise` filters an (H, W, 3) u8 image on its own, `chroma_denoise_yuv420` the U and
V planes of a planar YUV 4:2:0 image.
"""
from __future__ import annotations

import dataclasses

from . import _native, _u8_stage as _u8, types


@dataclasses.dataclass(frozen=True)
class ChromaDenoise:
    """The chroma noise filter.  radius (1, 2 or 3) is the window in cells of 2 x 2 pixels: 9, 25 or 49 taps; a tap counts
    when its cell's luma is within luma_threshold (0 .. 255 luma codes; 255 accepts every tap) and both its chroma
    differences within chroma_threshold (0 .. 255 codes) of the cell's own; strength (0 .. 1) is how far the chroma moves
    to the mean of those taps, quantised once to 1/64."""
    radius: int = 2
    luma_threshold: int = 8
    chroma_threshold: int = 12
    strength: float = 1.0

    def __post_init__(self):
        _u8.int_field("ChromaDenoise", "radius", self.radius, 1, 3)
        _u8.int_field("ChromaDenoise", "luma_threshold", self.luma_threshold, 0, 255)
        _u8.int_field("ChromaDenoise", "chroma_threshold", self.chroma_threshold, 0, 255)
        _u8.number("ChromaDenoise", "strength", self.strength, 0, 1)

    @property
    def strength_q6(self) -> int:
        """S = floor(strength * 64 + 0.5): the weight the filter multiplies with, 0 .. 64."""
        return _u8.q6(self.strength)

    def _arg(self) -> "_native.ChromaDenoise":
        """The mi_isp_chroma_denoise of these settings."""
        return _native.ChromaDenoise(int(self.radius), int(self.luma_threshold), int(self.chroma_threshold),
                                     self.strength_q6)


def check_chroma_denoise(value):
    """The ChromaDenoise of a constructor / set() argument, None for None; ValueError otherwise."""
    return _u8.check_setting(value, ChromaDenoise, "chroma_denoise")


def apply(images, settings: ChromaDenoise, yuv420=False):
    """New tensors holding the filter of the u8 device tensors `images` (one shape, contiguous, one device): (H, W, 3)
    images, or with yuv420 planar (H * 3 / 2, W) ones; one launch per 32 images (and one copy of the Y rows for the
    planar form) on the device's current stream, no host synchronisation."""
    return _u8.apply_batch(images, "mi_isp_chroma_denoise_rgb_batch", "mi_isp_chroma_denoise_yuv420_batch", settings._arg(),
                           yuv420)


def chroma_denoise(image, settings: ChromaDenoise):
    """The filter on an (H, W, 3) u8 RGB image: B - L and R - L of each 2 x 2 cell move toward their mean over the window's
    similar cells, G moves so that the luma stays (within a code, up to saturation).  numpy in gives numpy out, torch in
    gives torch out on the same device (a new tensor: the stencil cannot run in place).  DESIGN.md 3, "Chroma noise
    reduction"."""
    dev = _u8.checked(image, settings, ChromaDenoise, "chroma_denoise")
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    return types.from_device(apply([dev], settings)[0], image)


def chroma_denoise_yuv420(yuv, settings: ChromaDenoise):
    """The filter on a planar YUV 4:2:0 u8 image (H * 3 / 2, W; H and W even) as color.split_yuv_420 reads it: the cells are
    the chroma samples, SL the sum of a cell's four Y, U and V move toward their means, and the Y rows come back unchanged.
    This is NOT the YUV image of the RGB result: Cb and Cr are scaled differences, B - L and R - L are not.  Containers as
    chroma_denoise."""
    dev = _u8.checked(yuv, settings, ChromaDenoise, "chroma_denoise_yuv420")
    assert dev.ndim == 2 and dev.shape[0] % 3 == 0 and dev.shape[1] % 2 == 0, "yuv must be (H * 3 / 2, W) with H, W even"
    return types.from_device(apply([dev], settings, yuv420=True)[0], yuv)
