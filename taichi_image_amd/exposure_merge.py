"""Exposure merge (an extension): the frames of an exposure bracket - one camera, one instant, the shortest exposure first,
known exposure ratios - become one linear raw frame in the units of the shortest.  Every long frame is weighted by its
inverse variance where it is usable, fades out towards saturation, and is dropped completely where it disagrees with the
shortest frame beyond the sensor's noise model (motion: no ghost).

`Camera16/32(exposure_merge=ExposureMerge(...))` runs it on every bracket the bracket loaders take (`load_packed12_bracket`
and its siblings), behind levels and in front of highlight reconstruction and the other raw stages; `merge_cfa` runs it on
normalised CFAs on its own.  DESIGN.md 3, "Exposure merge".
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

import numpy as np
import torch

from . import _native, types


def _number_f32(name, v):
    """v as a Python float and as its f32 value; ValueError unless it is a number that is finite, in f32 too."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"ExposureMerge.{name} must be a number, got {v!r}")
    f = float(v)
    f32 = float(np.float32(f)) if math.isfinite(f) and abs(f) < 3.4e38 else math.inf
    if not math.isfinite(f32):
        raise ValueError(f"ExposureMerge.{name} must be finite (in f32 too), got {v!r}")
    return f, f32


def _positive_f32(x):
    """x (a double) rounds to an f32 that is finite and > 0."""
    if not math.isfinite(x) or abs(x) >= 3.4e38:
        return False
    return float(np.float32(x)) > 0


@dataclasses.dataclass(frozen=True)
class ExposureMerge:
    """The exposure merge.  ratios: the E exposure ratios (2 <= E <= 4), ratios[0] == 1, strictly increasing, <= 65536;
    gain, read_noise: RawDenoise's noise model in the units of the shortest frame's x (1.0 = the white level);
    saturation: in the units of x, a long frame's value at or above it is not used; knee (0 < knee <= 1): the usable
    weight falls linearly from 1 at saturation * (1 - knee) to 0 at saturation; threshold: the mean absolute difference to
    the shortest frame, in noise standard deviations, at which a long frame is dropped completely."""
    ratios: tuple
    gain: float
    read_noise: float
    saturation: float = 0.9
    knee: float = 0.25
    threshold: float = 4.0

    def __post_init__(self):
        if isinstance(self.ratios, (str, bytes)) or not isinstance(self.ratios, (tuple, list, np.ndarray)):
            raise ValueError(f"ExposureMerge.ratios must be a sequence of 2 to 4 numbers, got {self.ratios!r}")
        if isinstance(self.ratios, np.ndarray) and self.ratios.ndim != 1:
            raise ValueError(f"ExposureMerge.ratios must be a sequence of 2 to 4 numbers, got shape {self.ratios.shape}")
        ratios = tuple(self.ratios)
        if not 2 <= len(ratios) <= 4:
            raise ValueError(f"ExposureMerge.ratios must hold 2 to 4 exposures, got {len(ratios)}")
        r32 = [_number_f32(f"ratios[{i}]", q)[1] for i, q in enumerate(ratios)]
        if r32[0] != 1.0:
            raise ValueError(f"ExposureMerge.ratios[0] must be 1 (the shortest exposure first), got {ratios[0]!r}")
        for i in range(1, len(r32)):
            if not (r32[i] > r32[i - 1] and r32[i] <= 65536.0):
                raise ValueError(f"ExposureMerge.ratios must increase strictly (in f32 too) and stay <= 65536, got {ratios!r}")
        object.__setattr__(self, "ratios", tuple(float(q) for q in ratios))
        _, g = _number_f32("gain", self.gain)
        if not g >= 0:
            raise ValueError(f"ExposureMerge.gain must be >= 0, got {self.gain!r}")
        for name in ("read_noise", "threshold"):
            f, v = _number_f32(name, getattr(self, name))
            if not (f > 0 and v > 0 and _positive_f32(v * v)):  # (the library squares the f32 value)
                raise ValueError(f"ExposureMerge.{name} must be > 0 with a square that is finite and > 0 in f32, "
                                 f"got {getattr(self, name)!r}")
        _, sat = _number_f32("saturation", self.saturation)
        if not sat > 0:
            raise ValueError(f"ExposureMerge.saturation must be > 0 (in f32 too), got {self.saturation!r}")
        _, knee = _number_f32("knee", self.knee)
        if not 0 < knee <= 1:
            raise ValueError(f"ExposureMerge.knee must be in (0, 1] (in f32 too), got {self.knee!r}")
        if not (sat * knee > 0 and _positive_f32(1.0 / (sat * knee))):
            raise ValueError(f"ExposureMerge: 1 / (saturation * knee) must be finite and > 0 in f32, got saturation "
                             f"{self.saturation!r}, knee {self.knee!r}")

    @property
    def exposures(self) -> int:
        """E, the number of frames of a bracket."""
        return len(self.ratios)

    def _arg(self) -> "_native.ExposureMerge":
        """The mi_isp_exposure_merge of these settings."""
        r = list(self.ratios) + [0.0] * (4 - len(self.ratios))
        return _native.ExposureMerge(len(self.ratios), (ctypes.c_float * 4)(*r), float(self.gain), float(self.read_noise),
                                     float(self.saturation), float(self.knee), float(self.threshold))


def check_exposure_merge(value):
    """The ExposureMerge of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, ExposureMerge):
        return value
    raise ValueError(f"exposure_merge must be None or an ExposureMerge, got {type(value).__name__}")


def check_bracket(frames, settings: ExposureMerge, what="bracket"):
    """The frames of one bracket as a list: ValueError unless it holds E tensors of one shape, dtype and device (nothing
    is uploaded or launched)."""
    if not isinstance(frames, (list, tuple)):
        raise ValueError(f"{what} must be a list of {settings.exposures} frames (the shortest exposure first), got "
                         f"{type(frames).__name__}")
    if len(frames) != settings.exposures:
        raise ValueError(f"{what} holds {len(frames)} frames, exposure_merge has {settings.exposures} ratios")
    f0 = frames[0]
    for e, f in enumerate(frames):
        if not isinstance(f, torch.Tensor):
            raise TypeError(f"{what}: frame {e} must be a torch.Tensor")
        if f.shape != f0.shape or f.dtype != f0.dtype or f.device != f0.device:
            raise ValueError(f"{what}: frame {e} is {tuple(f.shape)} {f.dtype} on {f.device}, frame 0 is "
                             f"{tuple(f0.shape)} {f0.dtype} on {f0.device}: the frames of a bracket share them")
    return list(frames)


def merge_cfa(cfas, settings: ExposureMerge):
    """The merge of E normalised (H, W) f16 or f32 CFAs (x_e = their values, the shortest exposure first; no levels, gain
    or defects): same dtype out.  numpy in gives numpy out, torch in gives torch out on the same device (DESIGN.md 3,
    "Exposure merge")."""
    if not isinstance(settings, ExposureMerge):
        raise ValueError(f"settings must be an ExposureMerge, got {type(settings).__name__}")
    if not isinstance(cfas, (list, tuple)) or len(cfas) != settings.exposures:
        raise ValueError(f"merge_cfa takes a list of {settings.exposures} CFAs (one per ratio)")
    c0 = cfas[0]
    dt = types.ti_type(c0)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"merge_cfa takes f16 or f32 CFAs, got {dt}")
    if c0.ndim != 2:
        raise ValueError("cfas must be (H, W)")
    for e, c in enumerate(cfas):
        if type(c) is not type(c0) or c.shape != c0.shape or c.dtype != c0.dtype or (
                isinstance(c, torch.Tensor) and c.device != c0.device):
            raise ValueError(f"merge_cfa: CFA {e} differs from CFA 0 in type, shape, dtype or device")
    device = c0.device if isinstance(c0, torch.Tensor) and c0.is_cuda else types.default_device()
    devs = [types.to_device(c, device).contiguous() for c in cfas]
    H, W = devs[0].shape
    out = torch.empty_like(devs[0])
    if H * W:
        _native.check(_native.lib().mi_isp_merge_cfa(_native.ptr_array(devs), out.data_ptr(), H, W, dt.code,
                                                     settings._arg(), _native.stream_ptr(out.device)))
    return types.from_device(out, c0)
