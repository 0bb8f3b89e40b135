"""Temporal noise reduction (an extension): every raw pixel is averaged with the same camera's previous output where the
scene has not moved, and returned untouched where it has (motion-adaptive, no motion compensation).

`Camera16/32(temporal_denoise=TemporalDenoise(...))` runs it on every raw frame the loaders take, after levels, highlight
reconstruction and chromatic aberration and before raw noise reduction, shading and the cast; the state of one camera is a
`TemporalHistory` that the caller passes as `history=`.  `temporal_cfa` runs it on a normalised CFA on its own.
DESIGN.md 3, "Temporal noise reduction".
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _native, types


def _number_f32(name, v):
    """v as a Python float and as its f32 value; ValueError unless it is a number that is finite, in f32 too."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"TemporalDenoise.{name} must be a number, got {v!r}")
    f = float(v)
    f32 = float(np.float32(f)) if math.isfinite(f) and abs(f) < 3.4e38 else math.inf
    if not math.isfinite(f32):
        raise ValueError(f"TemporalDenoise.{name} must be finite (in f32 too), got {v!r}")
    return f, f32


@dataclasses.dataclass(frozen=True)
class TemporalDenoise:
    """The temporal filter.  gain, read_noise: RawDenoise's noise model in the units of the loader's x (1.0 = the white
    level); threshold: the mean absolute frame difference, in noise standard deviations, at which the past is dropped
    completely; max_weight: the weight of the past on a static pixel (0 <= max_weight < 1)."""
    gain: float
    read_noise: float
    threshold: float = 3.0
    max_weight: float = 0.75

    def __post_init__(self):
        _, g = _number_f32("gain", self.gain)
        if not g >= 0:
            raise ValueError(f"TemporalDenoise.gain must be >= 0, got {self.gain!r}")
        for name in ("read_noise", "threshold"):
            f, v = _number_f32(name, getattr(self, name))
            sq = float(np.float32(v * v)) if abs(v) < 1e19 else math.inf       # (the library squares the f32 value)
            if not (f > 0 and v > 0 and math.isfinite(sq) and sq > 0):
                raise ValueError(f"TemporalDenoise.{name} must be > 0 with a square that is finite and > 0 in f32, "
                                 f"got {getattr(self, name)!r}")
        _, w = _number_f32("max_weight", self.max_weight)
        if not 0 <= w < 1:
            raise ValueError(f"TemporalDenoise.max_weight must be in [0, 1) (in f32 too), got {self.max_weight!r}")

    def _arg(self) -> "_native.Temporal":
        """The mi_isp_temporal of these settings."""
        return _native.Temporal(float(self.gain), float(self.read_noise), float(self.threshold), float(self.max_weight))


def check_temporal_denoise(value):
    """The TemporalDenoise of a constructor / set() argument, None for None; ValueError otherwise."""
    if value is None or isinstance(value, TemporalDenoise):
        return value
    raise ValueError(f"temporal_denoise must be None or a TemporalDenoise, got {type(value).__name__}")


class TemporalHistory:
    """The state of one camera's temporal filter: two (H, W) f32 device planes - the history (the filter's previous
    output y) and the one the next frame writes - allocated on first use, and the frame shape and device they belong to.
    A loader reads `plane`, writes the other and swaps them once the launch was issued without error.  reset() empties
    the history (the next frame is a first frame: y = x); the planes stay allocated.  One object per camera: frames of
    another camera, shape or device are rejected, not mixed."""

    def __init__(self):
        self._planes = None                                  # [history, spare] once allocated
        self._shape = None
        self._device = None
        self._valid = False                                  # the history plane holds a frame
        self._frames = 0

    @property
    def frames(self) -> int:
        """The frames filtered into this history since it was created or reset (read-only)."""
        return self._frames

    @property
    def shape(self):
        """(H, W) of the frames this history belongs to, None before the first."""
        return self._shape

    @property
    def device(self):
        """The device of its planes, None before the first frame."""
        return self._device

    @property
    def plane(self):
        """The history plane, an (H, W) f32 device tensor (the filter's last y), or None while the history is empty."""
        return self._planes[0] if self._valid else None

    def reset(self):
        """Empty the history: the next frame is a first frame (a scene cut, new sensor levels, another exposure)."""
        self._valid = False
        self._frames = 0

    def _check(self, shape, device):
        """ValueError unless this history is new or belongs to frames of `shape` on `device` (nothing is changed)."""
        shape, device = (int(shape[0]), int(shape[1])), torch.device(device)
        if self._shape is not None and (self._shape != shape or self._device != device):
            raise ValueError(f"history= holds {self._shape[0]}x{self._shape[1]} frames on {self._device}, the frame is "
                             f"{shape[0]}x{shape[1]} on {device}: one TemporalHistory per camera (a new one, or reset() "
                             f"after which it still belongs to that shape and device)")

    def _begin(self, shape, device):
        """(the plane to read or None, the plane to write) for a frame of `shape` on `device`, allocating on first use."""
        self._check(shape, device)
        if self._planes is None:
            self._shape, self._device = (int(shape[0]), int(shape[1])), torch.device(device)
            self._planes = [torch.empty(self._shape, dtype=torch.float32, device=self._device) for _ in range(2)]
        return (self._planes[0] if self._valid else None), self._planes[1]

    def _commit(self):
        """The launch was issued: the written plane is the history."""
        self._planes.reverse()
        self._valid = True
        self._frames += 1


def check_history(value, shape, device):
    """The TemporalHistory of a history= entry, checked against the frame's shape and device; ValueError otherwise."""
    if not isinstance(value, TemporalHistory):
        raise ValueError(f"history= takes a TemporalHistory per frame, got {type(value).__name__}: pass history=")
    value._check(shape, device)
    return value


def check_histories(temporal, values, n, shape, device):
    """The histories of a loader call with n frames (values: None or a list of n), checked before anything is uploaded or
    launched: None when the stage is off (a history= is then a ValueError), else one distinct TemporalHistory per frame of
    the frames' shape and device.  RuntimeError while the device's current stream is being captured: the two planes
    alternate, so a replay would read the wrong one."""
    if temporal is None:
        if values is not None:
            raise ValueError("history= was given but temporal_denoise is off")
        return None
    if values is None or len(values) != n or any(v is None for v in values):
        raise ValueError(f"temporal_denoise is on: pass history= with one TemporalHistory per frame ({n})")
    hs = [check_history(v, shape, device) for v in values]
    if len({id(h) for h in hs}) != len(hs):
        raise ValueError("history= holds the same TemporalHistory twice: one per camera")
    if torch.device(device).type == "cuda" and torch.cuda.is_available():
        with torch.cuda.device(device):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("temporal_denoise cannot be captured into a graph: a history's two planes alternate, "
                                   "so a replay would read the wrong one")
    return hs


def temporal_cfa(cfa, history: TemporalHistory, settings: TemporalDenoise):
    """The filter on a normalised (H, W) f16 or f32 CFA (x = its values, no levels, gain or defects) against `history`,
    which it advances: same dtype out.  numpy in gives numpy out, torch in gives torch out on the same device (DESIGN.md 3,
    "Temporal noise reduction")."""
    if not isinstance(settings, TemporalDenoise):
        raise ValueError(f"settings must be a TemporalDenoise, got {type(settings).__name__}")
    if not isinstance(history, TemporalHistory):
        raise ValueError(f"history must be a TemporalHistory, got {type(history).__name__}")
    dt = types.ti_type(cfa)
    if dt not in (types.f16, types.f32):
        raise ValueError(f"temporal_cfa takes an f16 or f32 CFA, got {dt}")
    if cfa.ndim != 2:
        raise ValueError("cfa must be (H, W)")
    # a device CFA is filtered where it is, a host one on the history's device (the default one for a new history)
    if isinstance(cfa, torch.Tensor) and cfa.is_cuda:
        device = cfa.device
    else:
        device = history.device if history.device is not None else types.default_device()
    check_histories(settings, [history], 1, cfa.shape, device)      # (before anything is uploaded or launched)
    dev = types.to_device(cfa, device)
    H, W = dev.shape
    out = torch.empty_like(dev)
    if H * W:
        hin, hout = history._begin((H, W), dev.device)
        _native.check(_native.lib().mi_isp_temporal_cfa(
            dev.data_ptr(), None if hin is None else hin.data_ptr(), hout.data_ptr(), out.data_ptr(), H, W, dt.code,
            settings._arg(), _native.stream_ptr(dev.device)))
        history._commit()
    return types.from_device(out, cfa)
