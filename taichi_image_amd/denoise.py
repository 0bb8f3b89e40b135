"""Raw-domain noise reduction (an extension): an edge-preserving bilateral filter over same-site neighbours, adapted to
the sensor's noise model (variance = gain * x + read_noise**2 in the units of the loader's pre-cast value x).

`Camera16/32(raw_denoise=RawDenoise(...))` filters every raw frame the loaders take before shading and the cast;
`denoise_cfa` filters a normalised CFA on its own; `noise_model_from_frames` fits the two noise numbers from a few frames
of a static scene.  DESIGN.md 3, "Raw noise reduction".
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _native, types


def _finite_f32(name, v, positive):
    """v as a Python float; ValueError unless it is a number that is finite in f32 and > 0 (positive) or >= 0."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"RawDenoise.{name} must be a number, got {v!r}")
    f = float(v)
    f32 = float(np.float32(f)) if math.isfinite(f) and abs(f) < 3.4e38 else math.inf
    if not math.isfinite(f32) or not (f32 > 0 if positive else f32 >= 0) or (positive and not f > 0):
        raise ValueError(f"RawDenoise.{name} must be finite and {'> 0' if positive else '>= 0'}, got {v!r}")
    return f


@dataclasses.dataclass(frozen=True)
class RawDenoise:
    """The raw noise filter.  gain, read_noise: the noise model in the units of the loader's x (1.0 = the white level);
    strength scales the edge threshold (the range kernel's width in noise standard deviations); radius 1 or 2 takes the
    8 or 24 same-site neighbours of a 5 x 5 or 9 x 9 raw window; spatial_sigma is the spatial kernel's width in site
    steps."""
    gain: float
    read_noise: float
    strength: float = 1.0
    radius: int = 1
    spatial_sigma: float = 1.0

    def __post_init__(self):
        _finite_f32("gain", self.gain, positive=False)
        for name in ("read_noise", "strength", "spatial_sigma"):
            _finite_f32(name, getattr(self, name), positive=True)
        if isinstance(self.radius, bool) or not isinstance(self.radius, (int, np.integer)) or self.radius not in (1, 2):
            raise ValueError(f"RawDenoise.radius must be 1 or 2, got {self.radius!r}")

    def _arg(self) -> "_native.Denoise":
        """The mi_isp_denoise of these settings."""
        return _native.Denoise(float(self.gain), float(self.read_noise), float(self.strength), float(self.spatial_sigma),
                               int(self.radius))


def check_raw_denoise(value):
    """The RawDenoise of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, RawDenoise):
        return value
    raise ValueError(f"raw_denoise must be None or a RawDenoise, got {type(value).__name__}")


def denoise_cfa(cfa, denoise: RawDenoise):
    """The filter on a normalised (H, W) f16 or f32 CFA (x = its values, no levels, gain or defects), same dtype out.
    numpy in gives numpy out, torch in gives torch out on the same device ("Raw noise reduction")."""
    if not isinstance(denoise, RawDenoise):
        raise ValueError(f"denoise must be a RawDenoise, got {type(denoise).__name__}")
    dt = types.ti_type(cfa)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"denoise_cfa takes an f16 or f32 CFA, got {dt}")
    dev = types.to_device(cfa)
    assert dev.ndim == 2, "cfa must be (H, W)"
    H, W = dev.shape
    out = torch.empty_like(dev)
    if H * W:
        _native.check(_native.lib().mi_isp_denoise_cfa(dev.data_ptr(), out.data_ptr(), H, W, dt.code, denoise._arg(),
                                                       _native.stream_ptr(dev.device)))
    return types.from_device(out, cfa)


def noise_model_from_frames(frames, bits=12, black_level=None, white_level=None, bins=64):
    """(gain, read_noise) of the noise model var = gain * x + read_noise**2 from K >= 2 raw frames of a static scene
    (calibration; NumPy, CPU).

    frames: (K, H, W) raw codes (numpy or torch; `packed.decode12(..., scaled=False)` gives them).  x of a code is the
    packed loaders' value: max(code - black_s, 0) / (white - black_s) per CFA site s = (row & 1) * 2 + (col & 1), white
    2**bits - 1 by default (load_16u's x with bits=16).  Per pixel the temporal mean and unbiased variance of x; pixels
    clipped at 0 or at the white level in any frame are dropped.  Per site the pixels are binned by mean (`bins` equal
    bins over the site's range), and the bins of every site (at least 8 pixels each) are fitted together by least squares
    weighted by count / variance**2 (the inverse variance of a sample variance).  A scene with a spread of brightness
    (a gradient, a chart) constrains both numbers; a negative intercept gives a tiny read_noise."""
    f = np.asarray(frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else frames)
    if f.ndim != 3 or f.shape[0] < 2:
        raise ValueError(f"frames must be (K, H, W) with K >= 2, got shape {f.shape}")
    _, H, W = f.shape
    top = (1 << int(bits)) - 1
    white = top if white_level is None else int(white_level)
    black = list(black_level) if isinstance(black_level, (list, tuple, np.ndarray)) else [black_level or 0] * 4
    if len(black) != 4 or not all(0 <= int(b) < white <= top for b in black):
        raise ValueError(f"levels must satisfy 0 <= black < white <= {top}, got black {black_level}, white {white_level}")
    ms, vs, ns = [], [], []
    for s in range(4):
        c = f[:, s >> 1::2, s & 1::2].astype(np.float64)
        x = np.maximum(c - int(black[s]), 0) / float(white - int(black[s]))
        ok = (x > 0).all(axis=0) & (c < white).all(axis=0)
        if not ok.any():
            continue
        m = x.mean(axis=0)[ok]
        v = x.var(axis=0, ddof=1)[ok]
        edges = np.linspace(m.min(), m.max(), int(bins) + 1)
        idx = np.clip(np.searchsorted(edges, m, side="right") - 1, 0, int(bins) - 1)
        n = np.bincount(idx, minlength=int(bins))
        keep = n >= 8
        ms.append((np.bincount(idx, m, minlength=int(bins)) / np.maximum(n, 1))[keep])
        vs.append((np.bincount(idx, v, minlength=int(bins)) / np.maximum(n, 1))[keep])
        ns.append(n[keep])
    m, v, n = (np.concatenate(a) if a else np.zeros(0) for a in (ms, vs, ns))
    if m.size < 2 or np.ptp(m) == 0:
        raise ValueError("noise_model_from_frames: the frames need unclipped pixels at two or more brightness levels")
    wts = n / np.maximum(v, 1e-30) ** 2
    A = np.stack([m, np.ones_like(m)], axis=1) * np.sqrt(wts)[:, None]
    (gain, rn2), *_ = np.linalg.lstsq(A, v * np.sqrt(wts), rcond=None)
    gain = max(float(gain), 0.0)
    read_noise = math.sqrt(rn2) if rn2 > 0 else float(np.sqrt(np.finfo(np.float32).tiny))
    return gain, read_noise
