"""Chroma noise reduction (an extension): a luma-guided mean of the chroma on the grid of 2 x 2 pixel cells of the u8 images
the tonemaps return, defined in integer arithmetic so that its output is the contract's bit for bit ("Chroma
noise reduction").

`Camera16/32(chroma_denoise=ChromaDenoise(...))` filters every u8 output of the tonemaps and of process_packed12, before
local contrast and sharpening; `chroma_denoise` filters an (H, W, 3) u8 image on its own, `chroma_denoise_yuv420` the U and
V planes of a planar YUV 4:2:0 image.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _native, types


def _int_field(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"ChromaDenoise.{name} must be an integer in {lo} .. {hi}, got {v!r}")


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
        _int_field("radius", self.radius, 1, 3)
        _int_field("luma_threshold", self.luma_threshold, 0, 255)
        _int_field("chroma_threshold", self.chroma_threshold, 0, 255)
        s = self.strength
        if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)):
            raise ValueError(f"ChromaDenoise.strength must be a number, got {s!r}")
        if not math.isfinite(float(s)) or not 0 <= float(s) <= 1:
            raise ValueError(f"ChromaDenoise.strength must be finite and within [0, 1], got {s!r}")

    @property
    def strength_q6(self) -> int:
        """S = floor(strength * 64 + 0.5): the weight the filter multiplies with, 0 .. 64."""
        return int(math.floor(float(self.strength) * 64 + 0.5))

    def _arg(self) -> "_native.ChromaDenoise":
        """The mi_isp_chroma_denoise of these settings."""
        return _native.ChromaDenoise(int(self.radius), int(self.luma_threshold), int(self.chroma_threshold),
                                     self.strength_q6)


def check_chroma_denoise(value):
    """The ChromaDenoise of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, ChromaDenoise):
        return value
    raise ValueError(f"chroma_denoise must be None or a ChromaDenoise, got {type(value).__name__}")


def apply(images, settings: ChromaDenoise, yuv420=False):
    """New tensors holding the filter of the u8 device tensors `images` (one shape, contiguous, one device): (H, W, 3)
    images, or with yuv420 planar (H * 3 / 2, W) ones; one launch per 32 images (and one copy of the Y rows for the planar
    form) on the device's current stream, no host synchronisation."""
    first = images[0]
    outs = [torch.empty_like(im) for im in images]
    if yuv420:
        H, W = first.shape[0] * 2 // 3, first.shape[1]
        fn = _native.lib().mi_isp_chroma_denoise_yuv420_batch
    else:
        H, W = first.shape[:2]
        fn = _native.lib().mi_isp_chroma_denoise_rgb_batch
    if H * W:
        _native.check(fn(_native.ptr_array(images), _native.ptr_array(outs), len(images), H, W, settings._arg(),
                         _native.stream_ptr(first.device)))
    return outs


def _checked(image, settings, what):
    if not isinstance(settings, ChromaDenoise):
        raise ValueError(f"settings must be a ChromaDenoise, got {type(settings).__name__}")
    if types.ti_type(image) != types.u8:
        raise ValueError(f"{what} takes a u8 image, got {types.ti_type(image)}")
    return types.to_device(image)


def chroma_denoise(image, settings: ChromaDenoise):
    """The filter on an (H, W, 3) u8 RGB image: B - L and R - L of each 2 x 2 cell move toward their mean over the window's
    similar cells, G moves so that the luma stays (within a code, up to saturation).  numpy in gives numpy out, torch in
    gives torch out on the same device (a new tensor: the stencil cannot run in place).  DESIGN.md 3, "Chroma noise
    reduction"."""
    dev = _checked(image, settings, "chroma_denoise")
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    return types.from_device(apply([dev], settings)[0], image)


def chroma_denoise_yuv420(yuv, settings: ChromaDenoise):
    """The filter on a planar YUV 4:2:0 u8 image (H * 3 / 2, W; H and W even) as color.split_yuv_420 reads it: the cells are
    the chroma samples, SL the sum of a cell's four Y, U and V move toward their means, and the Y rows come back unchanged.
    This is NOT the YUV image of the RGB result: Cb and Cr are scaled differences, B - L and R - L are not.  Containers as
    chroma_denoise."""
    dev = _checked(yuv, settings, "chroma_denoise_yuv420")
    assert dev.ndim == 2 and dev.shape[0] % 3 == 0 and dev.shape[1] % 2 == 0, "yuv must be (H * 3 / 2, W) with H, W even"
    return types.from_device(apply([dev], settings, yuv420=True)[0], yuv)
