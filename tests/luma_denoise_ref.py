"""Luma noise reduction as DESIGN.md 3 ("Luma noise reduction") states it, in NumPy integers.  It does not call the
library: the settings are plain arguments (radius, threshold t0, threshold_bright t1 - None: t0 -, strength; S =
floor(strength * 64 + 0.5)).  Three switches give the mutants the tests must tell from the contract; none is the contract."""
import math

import numpy as np

from tests import sharpen_ref

DEFAULTS = dict(radius=2, threshold=6, threshold_bright=None, strength=1.0)


def strength_q6(strength):
    return int(math.floor(strength * 64 + 0.5))


def thresholds(L, threshold, threshold_bright=None, fixed_threshold=False):
    """T per pixel of an (H, W) integer luma image: t0 + (((t1 - t0) L + 128) >> 8).  fixed_threshold=True ignores
    threshold_bright (NOT the contract)."""
    t0 = int(threshold)
    t1 = t0 if threshold_bright is None or fixed_threshold else int(threshold_bright)
    return t0 + (((t1 - t0) * L.astype(np.int64) + 128) >> 8)


def window(L, radius, T, clamp_border=False):
    """(n, s) per pixel: the count and the luma sum of the taps inside the image with |L(q) - L(p)| <= T(p).
    clamp_border=True clamps a tap outside the image to the edge pixel and counts it (NOT the contract, where it is no
    tap)."""
    L = L.astype(np.int64)
    H, W = L.shape
    r = radius
    P = np.pad(L, r, mode="edge" if clamp_border else "constant")
    inside = np.pad(np.ones((H, W), bool), r, mode="edge" if clamp_border else "constant")
    n = np.zeros((H, W), np.int64)
    s = np.zeros((H, W), np.int64)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            q = P[i:i + H, j:j + W]
            ok = inside[i:i + H, j:j + W] & (np.abs(q - L) <= T)
            n += ok
            s += np.where(ok, q, 0)
    return n, s


def delta(L, radius=2, threshold=6, threshold_bright=None, strength=1.0, clamp_border=False, truncate=False,
          fixed_threshold=False):
    """dl per pixel of an (H, W) integer luma image.  truncate=True divides and shifts toward zero (NOT the contract)."""
    L = np.asarray(L).astype(np.int64)
    S = strength_q6(strength)
    T = thresholds(L, threshold, threshold_bright, fixed_threshold)
    n, s = window(L, radius, T, clamp_border)
    if truncate:                                                    # d = m - L as C's (2 (s - n L) + n) / (2 n), dl as C's / 64
        dn = 2 * (s - n * L) + n
        d = np.sign(dn) * (np.abs(dn) // (2 * n))
        num = S * d + 32
        return np.sign(num) * (np.abs(num) >> 6)
    m = (2 * s + n) // (2 * n)
    return (S * (m - L) + 32) >> 6


def luma_denoise_rgb(img, radius=2, threshold=6, threshold_bright=None, strength=1.0, clamp_border=False, truncate=False,
                     fixed_threshold=False):
    """The operator on an (H, W, 3) u8 image."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    if img.size == 0:
        return img.copy()
    dl = delta(sharpen_ref.luma(img), radius, threshold, threshold_bright, strength, clamp_border, truncate, fixed_threshold)
    return np.clip(img.astype(np.int64) + dl[..., None], 0, 255).astype(np.uint8)


def luma_denoise_yuv420(yuv, radius=2, threshold=6, threshold_bright=None, strength=1.0, clamp_border=False,
                        truncate=False, fixed_threshold=False):
    """The operator on a planar (H * 3 / 2, W) u8 YUV 4:2:0 image, H and W even: the Y plane filtered with L = Y, the
    chroma rows as they are."""
    assert yuv.dtype == np.uint8 and yuv.ndim == 2 and yuv.shape[0] % 3 == 0 and yuv.shape[1] % 2 == 0
    out = yuv.copy()
    H, W = yuv.shape[0] * 2 // 3, yuv.shape[1]
    if H * W:
        assert H % 2 == 0
        y = yuv[:H].astype(np.int64)
        dl = delta(y, radius, threshold, threshold_bright, strength, clamp_border, truncate, fixed_threshold)
        out[:H] = np.clip(y + dl, 0, 255).astype(np.uint8)
    return out
