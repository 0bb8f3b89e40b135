"""Defective pixel correction: per-sensor defect maps for the ISP's raw loaders (an extension).

A DefectMap is a set D of raw pixel positions (row, col) of one H x W frame - hot, stuck or dead sites.  The loaders of
Camera16 / Camera32 take one per call (`defects=`), since one ISP meters a whole camera group but defects belong to one
sensor.  Every listed site reads the mean of its same-site neighbours at distance 2 (axial first, the diagonals when no
axial one is usable); the demosaic, colour matrix, resize and metering subsample see the corrected value.  The device
arrays (coordinates, a bit mask, the per-geometry output lists of the packed fix-up) are uploaded once per device and
cached on the map, so a call with a map that was used before makes no host-device copy and can be captured in a graph.

find_defects is the calibration helper: it finds the sites of a uniform exposure (dark frames: hot pixels; flats: dead
ones) that stand out of their neighbourhood.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _native

f32 = np.float32


class DefectMap:
    """A set of defective raw pixel positions of one (H, W) frame.

    coords: (N, 2) integers (row, col), each inside the frame; duplicates are dropped and the coordinates are sorted
    row-major.  shape: (H, W), both even and positive.  ValueError otherwise."""

    def __init__(self, coords, shape):
        if not (isinstance(shape, (tuple, list)) and len(shape) == 2):
            raise ValueError(f"shape must be (H, W), got {shape!r}")
        H, W = shape
        for v in (H, W):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"shape must hold integers, got {shape!r}")
        H, W = int(H), int(W)
        if H <= 0 or W <= 0 or H % 2 or W % 2:
            raise ValueError(f"shape {(H, W)} must be even and positive")
        if H * W >= 2 ** 31:
            raise ValueError(f"shape {(H, W)} has too many pixels")
        c = np.asarray(coords.detach().cpu().numpy() if isinstance(coords, torch.Tensor) else coords)
        if c.size == 0:
            c = np.zeros((0, 2), np.int64)
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError(f"coords must be (N, 2) (row, col), got shape {c.shape}")
        if c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"coords must be integers, got {c.dtype}")
        c = c.astype(np.int64)
        if len(c) and (c[:, 0].min() < 0 or c[:, 0].max() >= H or c[:, 1].min() < 0 or c[:, 1].max() >= W):
            raise ValueError(f"coords outside the {H} x {W} frame")
        lin = np.unique(c[:, 0] * W + c[:, 1])
        self._coords = np.stack([lin // W, lin % W], axis=1).astype(np.int32)
        self._coords.setflags(write=False)
        self._shape = (H, W)
        self._dev = {}                                   # device index -> {"coords", "mask", (Hd, Wd, scale): list}

    @classmethod
    def from_mask(cls, mask) -> "DefectMap":
        """The map of the True entries of a boolean (H, W) mask."""
        m = np.asarray(mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else mask)
        if m.ndim != 2 or m.dtype != np.bool_:
            raise ValueError(f"mask must be a boolean (H, W) array, got {m.dtype} {m.shape}")
        return cls(np.argwhere(m), m.shape)

    @property
    def coords(self) -> np.ndarray:
        """(N, 2) int32 (row, col), sorted row-major, read-only."""
        return self._coords

    @property
    def shape(self):
        return self._shape

    def __len__(self) -> int:
        return len(self._coords)

    def __repr__(self) -> str:
        return f"DefectMap({len(self)} sites, shape={self._shape})"

    def mask(self) -> np.ndarray:
        """The boolean (H, W) mask of the map."""
        m = np.zeros(self._shape, bool)
        m[self._coords[:, 0], self._coords[:, 1]] = True
        return m

    def mask_words(self) -> np.ndarray:
        """The bit mask the kernels test: H rows of ceil(W / 32) u32 words, bit (col & 31) of word col >> 5."""
        H, W = self._shape
        mw = (W + 31) // 32
        bits = np.zeros((H, mw * 32), bool)
        bits[:, :W] = self.mask()
        return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(H, mw)

    def affected_outputs(self, Hd: int, Wd: int, scale: float = 0.0) -> np.ndarray:
        """The sorted unique indices (row * Wd + col) of the output pixels whose value reads a listed site: the 5 x 5
        demosaic footprint of every site at full resolution (scale 0), or every pixel of the fused bilinear resize
        (interpolate.py:24-34, p = f32(i) / f32(scale), taps trunc(p) and trunc(p) + 1 clamped) with a tap in one."""
        H, W = self._shape
        if len(self) == 0:
            return np.zeros(0, np.int32)
        d = np.arange(-2, 3)
        rr = (self._coords[:, 0, None, None] + d[None, :, None]).repeat(5, axis=2).reshape(-1)
        cc = (self._coords[:, 1, None, None] + d[None, None, :]).repeat(5, axis=1).reshape(-1)
        ok = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
        if not scale > 0:
            assert (Hd, Wd) == (H, W), "without a resize the output is the frame"
            return np.unique(rr[ok].astype(np.int64) * W + cc[ok]).astype(np.int32)
        A = np.zeros((H, W), bool)
        A[rr[ok], cc[ok]] = True
        s = f32(scale)

        def taps(n_out, n_px):
            p = np.arange(n_out, dtype=np.int32).astype(f32) / s
            i = np.trunc(p).astype(np.int64)
            return np.minimum(i, n_px - 1), np.minimum(i + 1, n_px - 1)

        r0, r1 = taps(Hd, H)
        c0, c1 = taps(Wd, W)
        rows_hit, cols_hit = A.any(axis=1), A.any(axis=0)
        ci = np.nonzero(rows_hit[r0] | rows_hit[r1])[0]          # candidate output rows / columns
        cj = np.nonzero(cols_hit[c0] | cols_hit[c1])[0]
        if len(ci) == 0 or len(cj) == 0:
            return np.zeros(0, np.int32)
        R0, R1 = A[r0[ci]], A[r1[ci]]
        hit = R0[:, c0[cj]] | R0[:, c1[cj]] | R1[:, c0[cj]] | R1[:, c1[cj]]
        ii, jj = np.nonzero(hit)
        return (ci[ii].astype(np.int64) * Wd + cj[jj]).astype(np.int32)

    # ---- device arrays (uploaded once per device, cached) -----------------------------------------------------------
    def _device(self, device: torch.device) -> dict:
        key = device.index if device.index is not None else torch.cuda.current_device()
        d = self._dev.get(key)
        if d is None:
            with torch.cuda.device(key):
                coords = torch.from_numpy(self._coords.copy()).to(device)
                mask = torch.from_numpy(self.mask_words().view(np.int32)).to(device)
            d = {"coords": coords, "mask": mask}
            self._dev[key] = d
        return d

    def _arg(self, device: torch.device) -> "_native.Defects":
        """The mi_isp_defects of this map on `device` (its tensors stay referenced by the map)."""
        d = self._device(device)
        return _native.Defects(d["coords"].data_ptr(), len(self), d["mask"].data_ptr())

    def _outputs(self, device: torch.device, Hd: int, Wd: int, scale: float):
        """(device int32 tensor, count) of affected_outputs(Hd, Wd, scale) on `device`, cached per geometry."""
        d = self._device(device)
        key = (int(Hd), int(Wd), float(f32(scale)) if scale > 0 else 0.0)
        hit = d.get(key)
        if hit is None:
            lst = self.affected_outputs(Hd, Wd, scale)
            with torch.cuda.device(device):
                t = torch.from_numpy(lst).to(device) if len(lst) else torch.zeros(1, dtype=torch.int32, device=device)
            hit = (t, len(lst))
            d[key] = hit
        return hit


def check_defects(defects, shape):
    """None for no correction (None or an empty map), else the map; ValueError for a map of another frame shape."""
    if defects is None:
        return None
    if not isinstance(defects, DefectMap):
        raise ValueError(f"defects must be a DefectMap or None, got {type(defects).__name__}")
    if tuple(defects.shape) != tuple(shape):
        raise ValueError(f"defect map of a {defects.shape[0]} x {defects.shape[1]} frame given for a "
                         f"{shape[0]} x {shape[1]} frame")
    return defects if len(defects) else None


def find_defects(frames, threshold) -> DefectMap:
    """Defective sites of a (K, H, W) stack of raw codes from a uniform exposure (calibration; NumPy, CPU).

    Dark frames find hot pixels, flat fields dead ones.  A pixel is flagged when its temporal mean differs by more than
    `threshold` codes from the median of the temporal means of its same-site neighbours at distance 2 (the 8 of
    (r +- 2, c), (r, c +- 2), (r +- 2, c +- 2) that are inside the frame)."""
    f = np.asarray(frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else frames)
    if f.ndim == 2:
        f = f[None]
    if f.ndim != 3 or f.shape[0] < 1:
        raise ValueError(f"frames must be (K, H, W), got shape {f.shape}")
    if not float(threshold) >= 0:
        raise ValueError(f"threshold must be a non-negative number, got {threshold!r}")
    _, H, W = f.shape
    mean = f.astype(np.float64).mean(axis=0)
    pad = np.full((H + 4, W + 4), np.nan)
    pad[2:-2, 2:-2] = mean
    offs = [(-2, 0), (2, 0), (0, -2), (0, 2), (-2, -2), (-2, 2), (2, -2), (2, 2)]
    flagged = np.zeros((H, W), bool)
    for r0 in range(0, H, 256):                          # row bands bound the memory of the neighbour stack
        r1 = min(H, r0 + 256)
        nb = np.stack([pad[2 + r0 + dr:2 + r1 + dr, 2 + dc:2 + W + dc] for dr, dc in offs])
        with warnings.catch_warnings():                  # (a pixel of a frame under 3 x 3 has no neighbour: not flagged)
            warnings.simplefilter("ignore", RuntimeWarning)
            med = np.nanmedian(nb, axis=0)
        flagged[r0:r1] = np.abs(mean[r0:r1] - med) > float(threshold)
    return DefectMap.from_mask(flagged)
