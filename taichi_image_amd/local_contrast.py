"""Local contrast (an extension): contrast-limited adaptive histogram equalisation (CLAHE) of the luma of the u8 images the
tonemaps return, defined in integer arithmetic so that its output is the contract's bit for bit ("Local
contrast").

`Camera16/32(local_contrast=LocalContrast(...))` equalises every u8 output of the tonemaps and of process_packed12 (before
sharpening, when both are set); `clahe` runs the operator on an (H, W, 3) u8 image on its own, `clahe_yuv420` on the Y plane
of a planar YUV 4:2:0 image.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native, _u8_stage as _u8, types

MAX_TILES = 16
MAX_SIDE = 32768


@dataclasses.dataclass(frozen=True)
class LocalContrast:
    """The local contrast operator.  tiles (Ty, Tx), 1 .. 16 each, are the tile rows x tile columns of the image as the
    caller gets it; clip_limit (None, or 1 .. 64) caps a histogram bin at that many times the uniform share, quantised once
    to 1/256 (None: plain adaptive equalisation); strength (0 .. 1) blends between the input and the equalised luma,
    quantised once to 1/64."""
    tiles: Tuple[int, int] = (8, 8)
    clip_limit: Optional[float] = 2.0
    strength: float = 1.0

    def __post_init__(self):
        t = self.tiles
        if not isinstance(t, (tuple, list)) or len(t) != 2 or any(
                isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= MAX_TILES for v in t):
            raise ValueError(f"LocalContrast.tiles must be a pair of integers in 1 .. {MAX_TILES}, got {t!r}")
        object.__setattr__(self, "tiles", (int(t[0]), int(t[1])))
        if self.clip_limit is not None:
            _u8.number("LocalContrast", "clip_limit", self.clip_limit, 1, 64)
        _u8.number("LocalContrast", "strength", self.strength, 0, 1)

    @property
    def clip_q8(self) -> int:
        """C = floor(clip_limit * 256 + 0.5), 256 .. 16384; 0 for None."""
        return 0 if self.clip_limit is None else int(math.floor(float(self.clip_limit) * 256 + 0.5))

    @property
    def strength_q6(self) -> int:
        """S = floor(strength * 64 + 0.5), 0 .. 64."""
        return _u8.q6(self.strength)

    def _arg(self) -> "_native.LocalContrast":
        """The mi_isp_local_contrast of these settings."""
        return _native.LocalContrast(self.tiles[0], self.tiles[1], self.clip_q8, self.strength_q6)


def check_local_contrast(value):
    """The LocalContrast of a constructor / set() argument, None for None; ValueError otherwise."""
    return _u8.check_setting(value, LocalContrast, "local_contrast")


def check_shape(H, W, lc: LocalContrast):
    """ValueError for an H x W image (the Y plane of a YUV one) that the tile grid does not fit; empty images pass."""
    if H * W and (H < lc.tiles[0] or W < lc.tiles[1] or H > MAX_SIDE or W > MAX_SIDE):
        raise ValueError(f"local_contrast: a {H} x {W} image does not take {lc.tiles[0]} x {lc.tiles[1]} tiles "
                         f"(at least one pixel per tile, at most {MAX_SIDE} rows and columns)")


def apply(images, lc: LocalContrast, yuv420=False, inplace=False):
    """The operator on the u8 device tensors `images` (one shape, contiguous, one device): (H, W, 3) images, or with yuv420
    planar (H * 3 / 2, W) ones.  inplace=True overwrites and returns `images` (the apply step is pointwise once the LUTs
    exist), else new tensors come back.  Four launches per 32 images on the device's current stream, no host
    synchronisation; the workspace (1280 bytes per tile and image) comes from torch's allocator."""
    H, W = _u8.geometry(images[0], yuv420)
    check_shape(H, W, lc)
    arg = lc._arg()
    ws = None
    if H * W:
        nbytes = int(_native.lib().mi_isp_local_contrast_workspace_bytes(len(images), arg))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=images[0].device)    # (alive until the launches are queued)
    return _u8.apply_batch(images, "mi_isp_local_contrast_rgb_batch", "mi_isp_local_contrast_yuv420_batch", arg, yuv420,
                           inplace, (ws.data_ptr() if ws is not None else 0,))


def clahe(image, lc: LocalContrast):
    """The operator on an (H, W, 3) u8 RGB image: the same delta, computed on the luma, is added to R, G and B, so hue is
    kept up to saturation.  numpy in gives numpy out, torch in gives torch out on the same device (always a new array).
    DESIGN.md 3, "Local contrast"."""
    dev = _u8.checked(image, lc, LocalContrast, "clahe", "local_contrast")
    assert dev.ndim == 3 and dev.shape[2] == 3, "image must be (H, W, 3)"
    return types.from_device(apply([dev], lc)[0], image)


def clahe_yuv420(yuv, lc: LocalContrast):
    """The operator on a planar YUV 4:2:0 u8 image (H * 3 / 2, W) as color.rgb_yuv420_image makes it: the Y plane (H, W)
    is the luma, out = clamp(Y + delta, 0, 255), and the chroma rows come back unchanged.  This is NOT the YUV image of the
    RGB result: there the luma is (77, 150, 29) / 256 of RGB and the delta saturates per channel.  Containers as clahe."""
    dev = _u8.checked(yuv, lc, LocalContrast, "clahe_yuv420", "local_contrast")
    assert dev.ndim == 2 and dev.shape[0] % 3 == 0 and dev.shape[1] % 2 == 0, "yuv must be (H * 3 / 2, W) with H, W even"
    return types.from_device(apply([dev], lc, yuv420=True)[0], yuv)
