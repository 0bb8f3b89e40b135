"""NumPy f32 restatement of the chromatic aberration contract ("Chromatic aberration"), shared by the
chromatic tests.  Every intermediate is an np.float32 array and every operation rounds once, in the contract's order.

correct() is y of every raw pixel from the pre-shading, pre-cast values x; route_cfa() the work-dtype CFA the route hands
to the demosaic (before the defect fix-up); coverage() what a generated frame must show for a case to mean anything.
`ca` is anything with the fields red, blue, center, norm_radius (a ChromaticAberration, or Settings below)."""
import collections
import math

import numpy as np

from oracle import isp_oracle as O

f32 = np.float32
COLOURS = O.PIXEL_ORDER                                  # pattern -> the colour (0 R, 1 G, 2 B) of sites 0 .. 3
Settings = collections.namedtuple("Settings", "red blue center norm_radius", defaults=((1, 0, 0), (1, 0, 0), None, None))


def host_values(ca, H, W):
    """(cy, cx, iR2, d_red, d_blue): what the library rounds once from double to f32."""
    cy, cx = ((H - 1) / 2.0, (W - 1) / 2.0) if ca.center is None else (float(ca.center[0]), float(ca.center[1]))
    nr = math.hypot(H / 2.0, W / 2.0) if ca.norm_radius is None else float(ca.norm_radius)
    d = [(f32(float(k[0]) - 1.0), f32(float(k[1])), f32(float(k[2]))) for k in (ca.red, ca.blue)]
    return f32(cy), f32(cx), f32(1.0 / (nr * nr)), d[0], d[1]


def mix(u, v, t):
    return ((u * (f32(1) - t).astype(f32)).astype(f32) + (v * t).astype(f32)).astype(f32)


def _taps(H, W, r0, c0, cy, cx, iR2, d):
    """The sampling of the site plane of parity (r0, c0): (i, fr, j, fc) with i (nr, nc) int64, fr (nr, nc) f32, ..."""
    fr_ = np.arange(r0, H, 2).astype(f32)[:, None]
    fc_ = np.arange(c0, W, 2).astype(f32)[None, :]
    dy = (fr_ - cy).astype(f32)
    dx = (fc_ - cx).astype(f32)
    r2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
    q = (r2 * iR2).astype(f32)
    e = (d[0] + (q * (d[1] + (q * d[2]).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    vs = (fr_ + (dy * e).astype(f32)).astype(f32)
    us = (fc_ + (dx * e).astype(f32)).astype(f32)
    a = ((vs - f32(r0)).astype(f32) * f32(0.5)).astype(f32)
    b = ((us - f32(c0)).astype(f32) * f32(0.5)).astype(f32)
    fi, fj = np.floor(a), np.floor(b)
    return fi.astype(np.int64), (a - fi).astype(f32), fj.astype(np.int64), (b - fj).astype(f32)


def correct(x, pattern, ca, excluded=None):
    """y (H, W) f32.  x: (H, W) f32; excluded: (H, W) bool, the defect map's sites (never a tap), or None."""
    x = np.asarray(x)
    assert x.dtype == f32 and x.ndim == 2
    H, W = x.shape
    y = x.copy()
    if H * W == 0:
        return y
    cy, cx, iR2, d_red, d_blue = host_values(ca, H, W)
    listed = np.zeros((H, W), bool) if excluded is None else np.asarray(excluded, bool)
    for s in range(4):
        colour = COLOURS[pattern][s]
        r0, c0 = s >> 1, s & 1
        P = x[r0::2, c0::2]
        if colour == 1 or P.size == 0:
            continue
        M = listed[r0::2, c0::2]
        nr, nc = P.shape
        with np.errstate(all="ignore"):
            i, fr, j, fc = _taps(H, W, r0, c0, cy, cx, iR2, d_blue if colour == 2 else d_red)
            i0, i1 = np.clip(i, 0, nr - 1), np.clip(i + 1, 0, nr - 1)
            j0, j1 = np.clip(j, 0, nc - 1), np.clip(j + 1, 0, nc - 1)
            t = [P[i0, j0], P[i0, j1], P[i1, j0], P[i1, j1]]
            out = mix(mix(t[0], t[1], fc), mix(t[2], t[3], fc), fr)
            m = [M[i0, j0], M[i0, j1], M[i1, j0], M[i1, j1]]
            if np.any(m):
                omr, omc = (f32(1) - fr).astype(f32), (f32(1) - fc).astype(f32)
                w = [(omr * omc).astype(f32), (omr * fc).astype(f32), (fr * omc).astype(f32), (fr * fc).astype(f32)]
                S = np.zeros(P.shape, f32)
                N = np.zeros(P.shape, f32)
                have = np.zeros(P.shape, bool)
                for wk, tk, mk in zip(w, t, m):          # the order 00, 01, 10, 11; each sum starts from its first kept term
                    keep = ~mk
                    wx = (wk * tk).astype(f32)
                    S = np.where(keep, np.where(have, (S + wk).astype(f32), wk), S).astype(f32)
                    N = np.where(keep, np.where(have, (N + wx).astype(f32), wx), N).astype(f32)
                    have = have | keep
                renorm = np.where(have & (S > 0), (N / S).astype(f32), P)
                out = np.where(m[0] | m[1] | m[2] | m[3], renorm, out).astype(f32)
        y[r0::2, c0::2] = out
    return y


def route_cfa(x, pattern, ca, work, gain=None, excluded=None):
    """The route's CFA before the defect fix-up: cast_work(y * g), or cast_work(y) without a grid."""
    y = correct(x, pattern, ca, excluded)
    return O.cast_out(y if gain is None else (y * np.asarray(gain, f32)).astype(f32), work)


def red_blue(pattern, H, W):
    """(H, W) bool: the red and blue sites."""
    s = (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)
    return np.asarray(COLOURS[pattern])[s] != 1


def coverage(x, pattern, ca):
    """Of the red / blue pixels of x, the fractions (whose first tap is a plane cell other than their own, with a tap
    clamped at the frame edge, that change among those that can, that cannot change).  A pixel cannot change when every
    tap of non-zero weight is its own cell: the pixel at the very centre of an odd-sized frame, and pixels whose taps all
    clamp onto them (a corner sampled outwards, an edge pixel on one of the centre's axes)."""
    H, W = x.shape
    cy, cx, iR2, d_red, d_blue = host_values(ca, H, W)
    y = correct(x, pattern, ca)
    moved = clamped = total = 0
    fixed = np.zeros((H, W), bool)
    for s in range(4):
        colour = COLOURS[pattern][s]
        r0, c0 = s >> 1, s & 1
        nr, nc = x[r0::2, c0::2].shape
        if colour == 1 or nr * nc == 0:
            continue
        i, fr, j, fc = _taps(H, W, r0, c0, cy, cx, iR2, d_blue if colour == 2 else d_red)
        own_i, own_j = np.arange(nr)[:, None], np.arange(nc)[None, :]
        moved += int(((i != own_i) | (j != own_j)).sum())
        clamped += int(((i < 0) | (i + 1 > nr - 1) | (j < 0) | (j + 1 > nc - 1)).sum())
        total += nr * nc
        rows_own = (np.clip(i, 0, nr - 1) == own_i) & ((fr == 0) | (np.clip(i + 1, 0, nr - 1) == own_i))
        cols_own = (np.clip(j, 0, nc - 1) == own_j) & ((fc == 0) | (np.clip(j + 1, 0, nc - 1) == own_j))
        fixed[r0::2, c0::2] = rows_own & cols_own
    free = red_blue(pattern, H, W) & ~fixed
    return moved / total, clamped / total, float((y != x)[free].mean()), int(fixed.sum()) / total


def frame_settings(H, W):
    """The settings of the generated-frame cases: a shift of 5.7 .. 5.8 px (red) and 4.8 .. 4.9 px (blue) at the corners."""
    Rn = math.hypot(H / 2.0, W / 2.0)
    return Settings((1 + 2 / Rn, 1.5 / Rn, 2.5 / Rn), (1 - 1 / Rn, -3 / Rn, -1 / Rn))

