"""Local tone mapping (an extension): every pixel of a linear work-dtype image times a gain that depends only on an
edge-aware local mean of its log-luminance, read from a bilateral grid (splat, blur, slice), in front of the global tone
curve.  Defined in integer and single f32 operations, so the output is the contract's bit for bit ("Local tone
mapping").  It is a tone control, not a radiometric one: the logarithm and the exponential are piecewise linear.

`Camera16/32(local_tonemap=LocalTonemap(...))` maps every image a loader returns; `local_tonemap` runs the operator on
(H, W, 3) f16 / f32 images on its own, `grids` returns the bilateral grid of one image.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _native, types

MAX_SIDE = 32768
CELLS = (8, 16, 32, 64)
MAX_BINS = 32
_F32_MIN_NORMAL = 2.0 ** -126


def _f32(name, v):
    """v as the f32 the library takes; ValueError for a bool, another type or a value that is not finite in f32."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"LocalTonemap.{name} must be a number, got {v!r}")
    with np.errstate(over="ignore"):
        f = float(np.float32(v))
    if not math.isfinite(f):
        raise ValueError(f"LocalTonemap.{name} must be finite in f32, got {v!r}")
    return f


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"LocalTonemap.{name} must be an integer, got {v!r}")
    return int(v)


def _li(t, floor):
    return (int(np.float32(t).view(np.int32)) - int(np.float32(floor).view(np.int32))) >> 12


@dataclasses.dataclass(frozen=True)
class LocalTonemap:
    """The local tone mapping operator.  strength (0 .. 1) is the share of the base layer's log-range that is removed;
    [floor, white] is the luminance range the logarithm covers (floor a normal f32, white / floor at most 2^24 and at
    least 2^-11 stops); anchor (floor .. white; None: white) is the luminance whose gain is 1 - with the default the
    highlights stay, the shadows are lifted and the gain is within [1, (white / floor)^strength]; cell (8, 16, 32 or 64) is
    the side of a grid cell in pixels, bins (2 .. 32) the number of log-luminance bins.  The values are taken as f32."""
    strength: float = 0.5
    white: float = 1.0
    floor: float = 2.0 ** -10
    anchor: Optional[float] = None
    cell: int = 32
    bins: int = 16

    def __post_init__(self):
        strength, white, floor = _f32("strength", self.strength), _f32("white", self.white), _f32("floor", self.floor)
        anchor = white if self.anchor is None else _f32("anchor", self.anchor)
        cell, bins = _int("cell", self.cell), _int("bins", self.bins)
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f"LocalTonemap.strength must be within [0, 1], got {self.strength!r}")
        if not white > 0.0:
            raise ValueError(f"LocalTonemap.white must be > 0, got {self.white!r}")
        if not _F32_MIN_NORMAL <= floor < white:
            raise ValueError(f"LocalTonemap.floor must be a normal f32 within (0, white), got {self.floor!r}")
        if white / floor > 2.0 ** 24:
            raise ValueError(f"LocalTonemap: white / floor = {white / floor} above 2**24")
        if _li(white, floor) < 1:
            raise ValueError(f"LocalTonemap: white {self.white!r} within 2**-11 stops of floor {self.floor!r}")
        if not floor <= anchor <= white:
            raise ValueError(f"LocalTonemap.anchor must be within [floor, white], got {self.anchor!r}")
        if cell not in CELLS:
            raise ValueError(f"LocalTonemap.cell must be one of {CELLS}, got {self.cell!r}")
        if not 2 <= bins <= MAX_BINS:
            raise ValueError(f"LocalTonemap.bins must be within 2 .. {MAX_BINS}, got {self.bins!r}")
        for name, v in (("strength", strength), ("white", white), ("floor", floor), ("anchor", anchor), ("cell", cell),
                        ("bins", bins)):
            object.__setattr__(self, name, v)

    def _arg(self) -> "_native.LocalTonemap":
        """The mi_isp_local_tonemap of these settings."""
        return _native.LocalTonemap(self.strength, self.white, self.floor, self.anchor, self.cell, self.bins)

    def grid_shape(self, H, W):
        """(GH, GW, bins) of the grid of an H x W image."""
        return (H + self.cell - 1) // self.cell, (W + self.cell - 1) // self.cell, self.bins


def check_local_tonemap(value):
    """The LocalTonemap of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, LocalTonemap):
        return value
    raise ValueError(f"local_tonemap must be None or a LocalTonemap, got {type(value).__name__}")


def check_shape(H, W):
    """ValueError for an image the operator does not take; empty images pass."""
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"local_tonemap: a {H} x {W} image has more than {MAX_SIDE} rows or columns")


_ws_cache: dict = {}


def _workspace(n, H, W, arg, device):
    """The workspace of a call on (device, current stream) for n images of H x W: cached, as _native.workspace (the passes
    write every entry they read, so its contents do not matter between calls)."""
    nbytes = int(_native.lib().mi_isp_local_tonemap_workspace_bytes(n, H, W, arg))
    key = (device.index or 0, int(_native.stream_ptr(device)), n, H, W, nbytes)
    ws = _ws_cache.get(key)
    if ws is None:
        if len(_ws_cache) > 64:
            _ws_cache.clear()
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def apply(images, settings: LocalTonemap):
    """The operator in place on the f16 / f32 device tensors `images` (H, W, 3), contiguous, one shape, dtype and device:
    ONE call of the library - three launches per 32 images on the device's current stream, no host synchronisation.
    Returns `images`."""
    if not images:
        return images
    first = images[0]
    H, W = first.shape[:2]
    check_shape(H, W)
    if H * W:
        arg = settings._arg()
        ws = _workspace(len(images), H, W, arg, first.device)
        _native.check(_native.lib().mi_isp_local_tonemap_batch(
            _native.ptr_array(images), len(images), H, W, types.ti_type(first).code, arg, ws.data_ptr(),
            _native.stream_ptr(first.device)))
    return images


def _checked(image, settings, what):
    if not isinstance(settings, LocalTonemap):
        raise ValueError(f"settings must be a LocalTonemap, got {type(settings).__name__}")
    dt = types.ti_type(image)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"{what} takes f16 or f32 images, got {dt}")
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"{what} takes (H, W, 3) images, got shape {tuple(image.shape)}")
    check_shape(*image.shape[:2])
    return dt


def local_tonemap(images, settings: LocalTonemap):
    """The operator on an (H, W, 3) f16 or f32 linear RGB image, or on a list of them (one shape and dtype; one call of the
    library for the list).  numpy in gives numpy out, torch in gives torch out on the same device; always new arrays.
    DESIGN.md 3, "Local tone mapping"."""
    single = not isinstance(images, (list, tuple))
    ims = [images] if single else list(images)
    for im in ims:
        _checked(im, settings, "local_tonemap")
        if im.shape != ims[0].shape or types.ti_type(im) != types.ti_type(ims[0]):
            raise ValueError("local_tonemap: the images of a call share a shape and a dtype")
    if not ims:
        return []
    device = next((im.device for im in ims if isinstance(im, torch.Tensor) and im.is_cuda), None)
    devs = []
    for im in ims:
        d = types.to_device(im, device)
        devs.append(d.clone() if isinstance(im, torch.Tensor) and d.data_ptr() == im.data_ptr() else d)
    apply(devs, settings)
    outs = [types.from_device(d, im) for d, im in zip(devs, ims)]
    return outs[0] if single else outs


def grids(image, settings: LocalTonemap):
    """(cnt, sum, Nb, Sb) of one (H, W, 3) f16 or f32 image: the splat counts and sums (uint32) and their blurred planes
    (f32), each (GH, GW, bins); the image is not written.  Containers as local_tonemap (numpy has uint32; torch planes of
    the counts come back as int32 holding the same bits)."""
    dt = _checked(image, settings, "grids")
    dev = types.to_device(image)
    H, W = dev.shape[:2]
    shape = settings.grid_shape(H, W)
    cnt, sm = (torch.zeros(shape, dtype=torch.int32, device=dev.device) for _ in range(2))
    nb, sb = (torch.zeros(shape, dtype=torch.float32, device=dev.device) for _ in range(2))
    if H * W:
        _native.check(_native.lib().mi_isp_local_tonemap_grids(
            dev.data_ptr(), H, W, dt.code, settings._arg(), cnt.data_ptr(), sm.data_ptr(), nb.data_ptr(), sb.data_ptr(),
            _native.stream_ptr(dev.device)))
    if isinstance(image, np.ndarray):
        return (cnt.cpu().numpy().view(np.uint32), sm.cpu().numpy().view(np.uint32), nb.cpu().numpy(), sb.cpu().numpy())
    return tuple(types.from_device(t, image) for t in (cnt, sm, nb, sb))
