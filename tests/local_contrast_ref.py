"""Local contrast (CLAHE on the luma) as DESIGN.md 3 ("Local contrast") states it, in NumPy integers.  It does not call
the library: the settings are plain arguments (tiles = (Ty, Tx), clip_limit None for no clip, strength 0 .. 1)."""
import math

import numpy as np

from tests.sharpen_ref import luma


def clip_q8(clip_limit):
    return 0 if clip_limit is None else int(math.floor(clip_limit * 256 + 0.5))


def strength_q6(strength):
    return int(math.floor(strength * 64 + 0.5))


def tile_bounds(M, T):
    """The T + 1 boundaries i M // T of an axis of M pixels."""
    return [i * M // T for i in range(T + 1)]


def redistribute(h, C, n):
    """The clipped histogram (int64[256]) of a tile of n pixels: the excess over c = max(1, (C n) >> 16) spread evenly,
    its residual e & 255 one count each to the bins 0, s, 2 s, ... with s = max(256 // r, 1)."""
    h = np.asarray(h).astype(np.int64).copy()
    if C:
        c = max(1, (C * n) >> 16)
        e = int(np.maximum(h - c, 0).sum())
        h = np.minimum(h, c) + (e >> 8)
        r = e & 255
        if r > 0:
            s = max(256 // r, 1)
            for k in range(r):
                h[k * s] += 1
    return h


def lut_of(h, n):
    """(2 * 255 * cdf + n) // (2 n) of a histogram with total n, int64[256]."""
    cdf = np.cumsum(np.asarray(h).astype(np.int64))
    return (2 * 255 * cdf + n) // (2 * n)


def histograms(L, tiles):
    """(Ty, Tx, 256) int64 histograms of an (H, W) integer luma image and the (Ty, Tx) pixel counts."""
    H, W = L.shape
    Ty, Tx = tiles
    ys, xs = tile_bounds(H, Ty), tile_bounds(W, Tx)
    hist = np.zeros((Ty, Tx, 256), np.int64)
    n = np.zeros((Ty, Tx), np.int64)
    for i in range(Ty):
        for j in range(Tx):
            t = L[ys[i]:ys[i + 1], xs[j]:xs[j + 1]]
            hist[i, j] = np.bincount(t.reshape(-1), minlength=256)
            n[i, j] = t.size
    return hist, n


def luts(L, tiles, clip_limit):
    """The (Ty, Tx, 256) int64 LUTs of an (H, W) integer luma image."""
    hist, n = histograms(L, tiles)
    C = clip_q8(clip_limit)
    out = np.zeros_like(hist)
    for i in range(tiles[0]):
        for j in range(tiles[1]):
            out[i, j] = lut_of(redistribute(hist[i, j], C, int(n[i, j])), int(n[i, j]))
    return out


def axis_weights(M, T):
    """(a, b, w) of every position of an axis of M pixels in T tiles: int64 arrays of M."""
    m = np.arange(M, dtype=np.int64)
    N = (2 * m + 1) * T - M
    i0 = N // (2 * M)                                               # floor: N may be negative
    rem = N - 2 * M * i0
    w = (256 * rem) // (2 * M)
    return np.clip(i0, 0, T - 1), np.clip(i0 + 1, 0, T - 1), w


def equalised(L, tiles, clip_limit):
    """E of an (H, W) integer luma image, int32 (every term fits: 256 * 256 * 255 + 32768 < 2^31)."""
    L = np.asarray(L).astype(np.int32)
    H, W = L.shape
    lut = luts(L, tiles, clip_limit).astype(np.int32).reshape(-1)
    ay, by, wy = (v[:, None].astype(np.int32) for v in axis_weights(H, tiles[0]))
    ax, bx, wx = (v[None, :].astype(np.int32) for v in axis_weights(W, tiles[1]))

    def at(i, j):                                                   # lut[i][j][L]
        return lut[(i * tiles[1] + j) * 256 + L]
    top = (256 - wx) * at(ay, ax) + wx * at(ay, bx)
    bot = (256 - wx) * at(by, ax) + wx * at(by, bx)
    return ((256 - wy) * top + wy * bot + 32768) >> 16


def blend(E, L, strength=1.0, truncate=False):
    """delta = ((E - L) S + 32) >> 6, int32.  truncate=True divides toward zero (NOT the contract: the mutation the tests
    must tell from it)."""
    num = (np.asarray(E).astype(np.int32) - np.asarray(L).astype(np.int32)) * strength_q6(strength) + 32
    if truncate:
        return np.sign(num) * (np.abs(num) >> 6)
    return num >> 6


def delta(L, tiles=(8, 8), clip_limit=2.0, strength=1.0, truncate=False):
    """The delta of an (H, W) integer luma image."""
    return blend(equalised(L, tiles, clip_limit), L, strength, truncate)


def add_rgb(img, dl):
    """clamp(I_c + delta, 0, 255) of an (H, W, 3) u8 image and its (H, W) deltas."""
    return np.clip(img.astype(np.int16) + dl[..., None].astype(np.int16), 0, 255).astype(np.uint8)


def add_yuv420(yuv, dl):
    """The planar (H * 3 / 2, W) image with the (H, W) deltas added to its Y plane, the chroma rows as they are."""
    out = yuv.copy()
    H = dl.shape[0]
    out[:H] = np.clip(yuv[:H].astype(np.int16) + dl.astype(np.int16), 0, 255).astype(np.uint8)
    return out


def clahe_rgb(img, tiles=(8, 8), clip_limit=2.0, strength=1.0, truncate=False):
    """The operator on an (H, W, 3) u8 image."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    if img.size == 0:
        return img.copy()
    return add_rgb(img, delta(luma(img), tiles, clip_limit, strength, truncate))


def clahe_yuv420(yuv, tiles=(8, 8), clip_limit=2.0, strength=1.0, truncate=False):
    """The operator on a planar (H * 3 / 2, W) u8 YUV 4:2:0 image: the Y plane equalised, the chroma rows as they are."""
    assert yuv.dtype == np.uint8 and yuv.ndim == 2 and yuv.shape[0] % 3 == 0
    H = yuv.shape[0] * 2 // 3
    if H * yuv.shape[1] == 0:
        return yuv.copy()
    return add_yuv420(yuv, delta(yuv[:H], tiles, clip_limit, strength, truncate))
