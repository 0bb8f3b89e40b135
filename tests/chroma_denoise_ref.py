"""Chroma noise reduction as DESIGN.md 3 ("Chroma noise reduction") states it, in NumPy integers.  It does not call the
library: the settings are plain arguments (radius, luma_threshold tl, chroma_threshold tc, strength; S = floor(strength *
64 + 0.5)).  Two switches give the mutants the tests must tell from the contract; neither is the contract."""
import math

import numpy as np

from tests import sharpen_ref

DEFAULTS = dict(radius=2, luma_threshold=8, chroma_threshold=12, strength=1.0)


def strength_q6(strength):
    return int(math.floor(strength * 64 + 0.5))


def _cell_sum(plane):
    """The sums over the 2 x 2 cells of an (H, W) integer plane, the last row / column counted twice at an odd edge."""
    H, W = plane.shape
    p = np.pad(plane.astype(np.int64), ((0, H & 1), (0, W & 1)), mode="edge")
    return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]


def cells_rgb(img):
    """(SL, SB, SR) of an (H, W, 3) u8 image, each (Hc, Wc) int64: the cell sums of the luma, of B - L and of R - L."""
    c = img.astype(np.int64)
    SL = _cell_sum(sharpen_ref.luma(img))
    return SL, _cell_sum(c[..., 2]) - SL, _cell_sum(c[..., 0]) - SL


def cells_yuv420(yuv):
    """(SL, SB, SR) of a planar (H * 3 / 2, W) u8 image: the cell sums of Y, 4 U and 4 V."""
    H, W = yuv.shape[0] * 2 // 3, yuv.shape[1]
    uv = yuv[H:].reshape(2, H // 2, W // 2).astype(np.int64)
    return _cell_sum(yuv[:H]), 4 * uv[0], 4 * uv[1]


def window(SL, SB, SR, radius, tl, tc, clamp_border=False):
    """(n, DB, DR) per cell: the count of the taps that pass and the sums of their SB - SB(p), SR - SR(p).
    clamp_border=True clamps a tap outside the grid to the edge cell (NOT the contract, where it is no tap)."""
    Hc, Wc = SL.shape
    r = radius
    mode = "edge" if clamp_border else "constant"
    P = [np.pad(a, r, mode=mode) for a in (SL, SB, SR)]
    inside = np.pad(np.ones((Hc, Wc), bool), r, mode="edge" if clamp_border else "constant")
    n = np.zeros((Hc, Wc), np.int64)
    DB = np.zeros((Hc, Wc), np.int64)
    DR = np.zeros((Hc, Wc), np.int64)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            ql, qb, qr = (a[i:i + Hc, j:j + Wc] for a in P)
            ok = (inside[i:i + Hc, j:j + Wc] & (np.abs(ql - SL) <= 4 * tl) & (np.abs(qb - SB) <= 4 * tc)
                  & (np.abs(qr - SR) <= 4 * tc))
            n += ok
            DB += np.where(ok, qb - SB, 0)
            DR += np.where(ok, qr - SR, 0)
    return n, DB, DR


def _div(num, den, truncate):
    if truncate:                                                    # C's num / den
        return np.sign(num) * (np.abs(num) // den)
    return num // den                                               # floor


def deltas(SL, SB, SR, radius=2, luma_threshold=8, chroma_threshold=12, strength=1.0, clamp_border=False,
           truncate=False):
    """(db, dr, dg) per cell.  truncate=True divides toward zero (NOT the contract)."""
    S = strength_q6(strength)
    n, DB, DR = window(SL, SB, SR, radius, luma_threshold, chroma_threshold, clamp_border)
    db = _div(2 * DB * S + 256 * n, 512 * n, truncate)
    dr = _div(2 * DR * S + 256 * n, 512 * n, truncate)
    dg = ((-(77 * dr + 29 * db)) * 437 + 32768) >> 16
    return db, dr, dg


def _per_pixel(d, H, W):
    return np.repeat(np.repeat(d, 2, axis=0), 2, axis=1)[:H, :W]


def chroma_denoise_rgb(img, radius=2, luma_threshold=8, chroma_threshold=12, strength=1.0, clamp_border=False,
                       truncate=False):
    """The operator on an (H, W, 3) u8 image."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    if img.size == 0:
        return img.copy()
    H, W = img.shape[:2]
    db, dr, dg = deltas(*cells_rgb(img), radius, luma_threshold, chroma_threshold, strength, clamp_border, truncate)
    d = np.stack([_per_pixel(x, H, W) for x in (dr, dg, db)], -1)
    return np.clip(img.astype(np.int64) + d, 0, 255).astype(np.uint8)


def chroma_denoise_yuv420(yuv, radius=2, luma_threshold=8, chroma_threshold=12, strength=1.0, clamp_border=False,
                          truncate=False):
    """The operator on a planar (H * 3 / 2, W) u8 YUV 4:2:0 image, H and W even: U and V filtered, the Y rows as they
    are."""
    assert yuv.dtype == np.uint8 and yuv.ndim == 2 and yuv.shape[0] % 3 == 0 and yuv.shape[1] % 2 == 0
    out = yuv.copy()
    H, W = yuv.shape[0] * 2 // 3, yuv.shape[1]
    if H * W:
        assert H % 2 == 0
        db, dr, _ = deltas(*cells_yuv420(yuv), radius, luma_threshold, chroma_threshold, strength, clamp_border, truncate)
        uv = yuv[H:].reshape(2, H // 2, W // 2).astype(np.int64)
        out[H:] = np.clip(uv + np.stack([db, dr]), 0, 255).astype(np.uint8).reshape(H // 2, W)
    return out


def scene_yuv420(rng, H, W):
    """The planar YUV 4:2:0 image (JPEG-range BT.601 matrix, chroma averaged over each 2 x 2 cell) of
    sharpen_ref.scene_u8, H and W even."""
    assert H % 2 == 0 and W % 2 == 0
    rgb = sharpen_ref.scene_u8(rng, H, W).astype(np.float64)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    U = -0.168736 * R - 0.331264 * G + 0.5 * B + 128.0
    V = 0.5 * R - 0.418688 * G - 0.081312 * B + 128.0
    avg = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4.0          # noqa: E731
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)                                   # noqa: E731
    return np.concatenate([q(Y).ravel(), q(avg(U)).ravel(), q(avg(V)).ravel()]).reshape(H * 3 // 2, W)
