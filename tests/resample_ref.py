"""The antialiased resize restated independently of the library ("Antialiased resize"): the table of an
axis in Python doubles, operation by operation in the contract's order, and the two f32 passes in NumPy with one rounding
per operation.  Nothing here imports the package.

`mutant=` switches one deliberate mistake on (the mutation record's operator-level twins): "reverse" (taps summed from
the last to the first), "f16_h" (the horizontal pass rounded to f16), "swap" (the two tables exchanged; square cases only).
"""
from __future__ import annotations

import math

import numpy as np

FILTERS = ("area", "triangle", "lanczos3")
MAX_TAPS = 32
f32 = np.float32


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    if x == float(round(x)):                 # (round half to even, as nearbyint: only the integers compare equal)
        return 0.0
    px = math.pi * x
    return math.sin(px) / px


def _taps_of(filt: str, s: float, d: int):
    """The (k, w) of output sample d in increasing k."""
    widen = 1.0 / s if s < 1.0 else 1.0
    c = d / s
    R = widen / 2.0 + 0.5 if filt == "area" else (widen if filt == "triangle" else 3.0 * widen)
    out = []
    for k in range(int(math.floor(c - R)), int(math.ceil(c + R)) + 1):
        if filt == "lanczos3":
            x = (k - c) / widen
            w = _sinc(x) * _sinc(x / 3.0) if abs(x) < 3.0 else 0.0
            tap = w != 0.0
        elif filt == "area" and s < 1.0:
            hi = min(k + 0.5, c + widen / 2.0)
            lo = max(k - 0.5, c - widen / 2.0)
            w = hi - lo
            tap = w > 0.0
        else:
            w = 1.0 - abs(k - c) / widen
            tap = w > 0.0
        if tap:
            out.append((k, w))
    return out


_cache: dict = {}


def table(filt: str, S: int, D: int, s: float, limit: bool = True):
    """(T, start int32[D], weight f32[D, T]) of the axis; ValueError beyond 32 taps unless limit=False."""
    assert filt in FILTERS
    key = (filt, S, D, float(s), limit)
    if key in _cache:
        return _cache[key]
    rows = [_taps_of(filt, float(s), d) for d in range(D)]
    T = min(max(r[-1][0] - r[0][0] + 1 for r in rows), S)
    if limit and T > MAX_TAPS:
        raise ValueError(f"{filt} at scale {s}: {T} taps")
    start = np.zeros(D, dtype=np.int32)
    weight = np.zeros((D, T), dtype=np.float32)
    for d, r in enumerate(rows):
        st = min(max(r[0][0], 0), S - T)
        acc = [0.0] * T
        for k, w in r:
            acc[min(max(k, 0), S - 1) - st] += w
        total = acc[0]
        for j in range(1, T):
            total = total + acc[j]
        start[d] = st
        weight[d] = [f32(a / total) for a in acc]
    _cache[key] = (T, start, weight)
    return _cache[key]


def _pass(x, start, weight, mutant=None):
    """Filter axis 1 of the f32 array x (rows, S, C): out[:, d] = the taps of d in order, one rounded multiply and one
    rounded add each; the first product starts the sum."""
    D, T = weight.shape
    order = range(T - 1, -1, -1) if mutant == "reverse" else range(T)
    acc = None
    with np.errstate(invalid="ignore", over="ignore"):
        for j in order:
            term = weight[:, j].astype(f32)[None, :, None] * x[:, start + j, :]
            acc = term if acc is None else (acc + term).astype(f32)
    return acc.astype(f32)


def resample(src, rows, cols, out_dtype=None, mutant=None):
    """The (Hs, Ws, 3) f16 / f32 image src through the tables rows = (Ty, sy, wy) and cols = (Tx, sx, wx): horizontal
    first into f32 (never rounded to f16), then vertical, then one cast to out_dtype (None: the source's)."""
    if mutant == "swap":
        rows, cols = cols, rows
    out_dtype = src.dtype if out_dtype is None else np.dtype(out_dtype)
    x = src.astype(f32)
    h = _pass(x, cols[1], cols[2], mutant)                            # (Hs, Wd, 3)
    if mutant == "f16_h":
        h = h.astype(np.float16).astype(f32)
    o = _pass(np.ascontiguousarray(h.transpose(1, 0, 2)), rows[1], rows[2], mutant).transpose(1, 0, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(o).astype(out_dtype)


def resize(src, size, scale, filt, out_dtype=None):
    """The whole operator: size = (w, h), scale a scalar or (row, col), as interpolate.resample."""
    Hs, Ws = src.shape[:2]
    Wd, Hd = size
    s0, s1 = (scale, scale) if np.isscalar(scale) else scale
    return resample(src, table(filt, Hs, Hd, s0), table(filt, Ws, Wd, s1), out_dtype)


def bilinear(src, size, scale):
    """The point-sampled resize on an f32 image (the 2 x 2 bilinear of interpolate.resize_bilinear, in double): what
    the reference-only properties compare against."""
    Hs, Ws = src.shape[:2]
    Wd, Hd = size
    x = src.astype(np.float64)
    pr, pc = np.arange(Hd) / scale, np.arange(Wd) / scale
    ir, ic = np.floor(pr).astype(int), np.floor(pc).astype(int)
    fr, fc = (pr - ir)[:, None, None], (pc - ic)[None, :, None]
    r0, r1 = np.clip(ir, 0, Hs - 1), np.clip(ir + 1, 0, Hs - 1)
    c0, c1 = np.clip(ic, 0, Ws - 1), np.clip(ic + 1, 0, Ws - 1)
    y1 = x[r0][:, c0] * (1 - fr) + x[r1][:, c0] * fr
    y2 = x[r0][:, c1] * (1 - fr) + x[r1][:, c1] * fr
    return y1 * (1 - fc) + y2 * fc
