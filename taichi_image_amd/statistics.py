"""Frame statistics (an extension): what a hardware ISP's "3A statistics" unit reports about the raw frames - per zone and
CFA site the mean, the clipped and the dark fraction, per zone a focus measure (the squared same-site Laplacian of the
green pixels), per site a 256-bin histogram - measured on the value the loaders compute before shading, white balance and
the cast.  Everything is summed in integers on the device, so the result is exact and independent of the launch.

`Camera16/32(statistics=Statistics(...))` measures every raw frame the loaders take, as a side output
(`isp.frame_statistics`) that changes no image; `statistics_cfa` measures a normalised CFA on its own.  DESIGN.md 3,
"Frame statistics".
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

import numpy as np
import torch

from . import _native, types
from .bayer import BayerPattern

SITES, BINS, MAX_ZONES = 4, 256, 32
MAX_PIXELS = 1 << 26


def _f32_number(name, v, rule, ok):
    """v as a Python float; ValueError unless it is a number that is finite, as a double and in f32, and ok(its f32 value)."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    f = float(v)
    f32 = float(np.float32(f)) if math.isfinite(f) and abs(f) < 3.4e38 else math.inf
    if not math.isfinite(f32) or not ok(f32):
        raise ValueError(f"{name} must be {rule} (in f32 too), got {v!r}")
    return f


@dataclasses.dataclass(frozen=True)
class Statistics:
    """The measurement.  zones = (rows, columns) of the zone grid, 1 .. 32 each and no more than the frame has quads; a
    pixel is clipped when x >= clip and dark when x <= dark, x in the units of the loader's value (1.0 = the white level)."""
    zones: tuple = (8, 8)
    clip: float = 0.98
    dark: float = 1.0 / 64.0

    def __post_init__(self):
        z = self.zones
        if (not isinstance(z, (tuple, list)) or len(z) != 2
                or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) for n in z)
                or any(not 1 <= n <= MAX_ZONES for n in z)):
            raise ValueError(f"Statistics.zones must be two integers in 1 .. {MAX_ZONES}, got {z!r}")
        object.__setattr__(self, "zones", (int(z[0]), int(z[1])))
        _f32_number("Statistics.clip", self.clip, "finite and > 0", lambda f: f > 0)
        clip32 = float(np.float32(self.clip))
        _f32_number("Statistics.dark", self.dark, "finite, >= 0 and below clip", lambda f: 0 <= f < clip32)

    @property
    def words(self) -> int:
        """The int64 words of one frame's result."""
        return self.zones[0] * self.zones[1] * 18 + SITES * BINS

    def check_shape(self, shape) -> None:
        """ValueError unless a frame of `shape` (H, W) can be measured: even, at most 2^26 pixels and 65535 tile rows of 64,
        no more zones than quads per axis (an empty frame is measured as nothing)."""
        H, W = int(shape[0]), int(shape[1])
        if H * W == 0:
            return
        if H % 2 or W % 2:
            raise ValueError(f"statistics: frames must be even size, got {H}x{W}")
        if H * W > MAX_PIXELS or (H + 63) // 64 > 65535:
            raise ValueError(f"statistics: frame {H}x{W} is too large (at most 2^26 pixels and 65535 tile rows)")
        if self.zones[0] > H // 2 or self.zones[1] > W // 2:
            raise ValueError(f"statistics: zones {self.zones[0]}x{self.zones[1]} exceed the {H // 2}x{W // 2} quads of the frame")

    def _arg(self) -> "_native.Statistics":
        """The mi_isp_statistics of these settings."""
        return _native.Statistics(self.zones[0], self.zones[1], float(self.clip), float(self.dark))


def check_statistics(value):
    """The Statistics of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, Statistics):
        return value
    raise ValueError(f"statistics must be None or a Statistics, got {type(value).__name__}")


class FrameStatistics:
    """One frame's result: int64 views of the one device buffer the kernel wrote (nothing is read to the host here).
    zones (gh, gw, 4, 4): per zone and site (row & 1) * 2 + (col & 1) the count of valid pixels, the sum of their
    v = rint(clamp(x, 0, 1) * 65536), the clipped and the dark; focus (gh, gw, 2): the sum of the squared Laplacians L of
    the green pixels that qualify and their count; histogram (4, 256): per site, bin min(v >> 8, 255).  The helpers
    read the buffer when they are called (a host synchronisation) and compute in f64."""

    def __init__(self, buffer: torch.Tensor, settings: Statistics):
        gh, gw = settings.zones
        assert buffer.dtype == torch.int64 and buffer.ndim == 1 and buffer.numel() == settings.words
        self.settings = settings
        self.buffer = buffer
        self.zones = buffer[:gh * gw * 16].view(gh, gw, SITES, 4)
        self.focus = buffer[gh * gw * 16:gh * gw * 18].view(gh, gw, 2)
        self.histogram = buffer[gh * gw * 18:].view(SITES, BINS)

    def _ratio(self, k):
        z = self.zones.cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(z[..., 0] > 0, z[..., k] / z[..., 0], np.nan)

    def mean(self) -> np.ndarray:
        """(gh, gw, 4) f64: the mean of clamp(x, 0, 1) per zone and site, NaN where the zone has no valid pixel of the site."""
        return self._ratio(1) / 65536.0

    def clipped_fraction(self) -> np.ndarray:
        """(gh, gw, 4) f64: the clipped share of the valid pixels per zone and site, NaN where there is none."""
        return self._ratio(2)

    def dark_fraction(self) -> np.ndarray:
        """(gh, gw, 4) f64: the dark share of the valid pixels per zone and site, NaN where there is none."""
        return self._ratio(3)

    def sharpness(self) -> np.ndarray:
        """(gh, gw) f64: the mean squared Laplacian of the green pixels in x units, NaN where no pixel qualified."""
        f = self.focus.cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(f[..., 1] > 0, f[..., 0] / f[..., 1] / 2.0 ** 32, np.nan)

    def percentile(self, q, site=None) -> float:
        """The q-th percentile (0 .. 100) of the histogram of `site` (None: all four together), as the lower edge in x units
        of the first bin at which the cumulative count reaches q per cent of the pixels; NaN for an empty histogram."""
        if isinstance(q, bool) or not isinstance(q, (int, float, np.integer, np.floating)) or not 0 <= float(q) <= 100:
            raise ValueError(f"q must be a number in 0 .. 100, got {q!r}")
        if site is not None and (isinstance(site, bool) or not isinstance(site, (int, np.integer)) or not 0 <= site < SITES):
            raise ValueError(f"site must be None or 0 .. 3, got {site!r}")
        h = self.histogram.cpu().numpy()
        h = h.sum(axis=0) if site is None else h[site]
        total = int(h.sum())
        if total == 0:
            return math.nan
        k = int(np.searchsorted(np.cumsum(h).astype(np.float64), float(q) / 100.0 * total, side="left"))
        return min(k, BINS - 1) / float(BINS)


def measure_raw(srcs, h, w, kind, ids_format, pattern, levels, defects, settings: Statistics, device):
    """The statistics of the raw device frames srcs (one shape, source kind `kind` of _native.MI_RAW_*, levels a
    _native.Levels or None, defects one _native.Defects or None per frame): one launch per 32 frames on the device's current
    stream, one FrameStatistics per frame, views of one buffer.  Nothing is read to the host."""
    n = len(srcs)
    words = settings.words
    buf = (torch.zeros if h * w == 0 else torch.empty)((n, words), dtype=torch.int64, device=device)
    outs = (ctypes.c_void_p * n)(*[buf[i].data_ptr() for i in range(n)])
    maps = (ctypes.c_void_p * n)(*[None if d is None else ctypes.addressof(d) for d in defects])
    _native.check(_native.lib().mi_isp_statistics_raw_batch(
        _native.ptr_array(srcs), outs, n, h, w, kind, int(bool(ids_format)), pattern.value, levels, maps, settings._arg(),
        _native.stream_ptr(device)))
    return [FrameStatistics(buf[i], settings) for i in range(n)]


def statistics_cfa(cfa, pattern: BayerPattern, settings: Statistics = Statistics(), defects=None) -> FrameStatistics:
    """The statistics of a normalised (H, W) f16 or f32 CFA (numpy or torch) of even size under the Bayer pattern `pattern`
    (x = its values, no levels); defects: None or the defects.DefectMap of the sensor.  The result stays on the device
    ("Frame statistics")."""
    from . import defects as _defects
    if not isinstance(settings, Statistics):
        raise ValueError(f"settings must be a Statistics, got {type(settings).__name__}")
    if not isinstance(pattern, BayerPattern):
        raise ValueError(f"pattern must be a BayerPattern, got {type(pattern).__name__}")
    dt = types.ti_type(cfa)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"statistics_cfa takes an f16 or f32 CFA, got {dt}")
    dev = types.to_device(cfa)
    assert dev.ndim == 2, "cfa must be (H, W)"
    H, W = dev.shape
    settings.check_shape((H, W))
    dm = _defects.check_defects(defects, (H, W))
    arg = None if dm is None else dm._arg(dev.device)
    buf = (torch.zeros if H * W == 0 else torch.empty)(settings.words, dtype=torch.int64, device=dev.device)
    _native.check(_native.lib().mi_isp_statistics_cfa(dev.data_ptr(), buf.data_ptr(), H, W, dt.code, pattern.value, arg,
                                                      settings._arg(), _native.stream_ptr(dev.device)))
    return FrameStatistics(buf, settings)
