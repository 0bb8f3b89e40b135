"""Output sharpening as DESIGN.md 3 ("Output sharpening") states it, in NumPy integers on padded arrays.  It does not call
the library: the settings are plain arguments (amount_q6 = floor(amount * 64 + 0.5), overshoot None for no halo clamp)."""
import math

import numpy as np

TAPS = {1: (1, 2, 1), 2: (1, 4, 6, 4, 1)}


def amount_q6(amount):
    return int(math.floor(amount * 64 + 0.5))


def luma(rgb):
    """(77 R + 150 G + 29 B + 128) >> 8 of an (H, W, 3) u8 image, int32."""
    c = rgb.astype(np.int32)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def delta(L, amount, radius=1, threshold=0, overshoot=None, truncate=False):
    """The delta of an (H, W) integer luma image.  truncate=True divides toward zero (NOT the contract: the mutation the
    tests must tell from it)."""
    L = np.asarray(L).astype(np.int32)
    H, W = L.shape
    b = TAPS[radius]
    r = radius
    S = sum(b) ** 2
    k = 6 + int(math.log2(S))
    A = amount_q6(amount)
    P = np.pad(L, r, mode="edge")
    Bl = np.zeros((H, W), np.int32)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            Bl += b[i] * b[j] * P[i:i + H, j:j + W]
    d = S * L - Bl
    dc = np.sign(d) * np.maximum(np.abs(d) - threshold * S, 0)
    if truncate:                                                    # C's (A d' + half) / 2**k
        num = A * dc + (1 << (k - 1))
        dl = np.sign(num) * (np.abs(num) >> k)
    else:
        dl = (A * dc + (1 << (k - 1))) >> k
    if overshoot is not None:
        Q = np.pad(L, 1, mode="edge")
        win = np.stack([Q[i:i + H, j:j + W] for i in range(3) for j in range(3)])
        dl = np.clip(L + dl, win.min(0) - overshoot, win.max(0) + overshoot) - L
    return dl.astype(np.int32)


def sharpen_rgb(img, amount, radius=1, threshold=0, overshoot=None, truncate=False):
    """The filter of an (H, W, 3) u8 image."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    if img.size == 0:
        return img.copy()
    dl = delta(luma(img), amount, radius, threshold, overshoot, truncate)
    return np.clip(img.astype(np.int32) + dl[..., None], 0, 255).astype(np.uint8)


def sharpen_yuv420(yuv, amount, radius=1, threshold=0, overshoot=None):
    """The filter of a planar (H * 3 / 2, W) u8 YUV 4:2:0 image: the Y plane filtered, the chroma rows as they are."""
    assert yuv.dtype == np.uint8 and yuv.ndim == 2 and yuv.shape[0] % 3 == 0
    out = yuv.copy()
    H = yuv.shape[0] * 2 // 3
    if H * yuv.shape[1]:
        y = yuv[:H].astype(np.int32)
        out[:H] = np.clip(y + delta(y, amount, radius, threshold, overshoot), 0, 255).astype(np.uint8)
    return out


def scene_u8(rng, H, W, sigma=0.03):
    """The smooth-plus-noise scene of tests/util.natural_packed12, as an (H, W, 3) u8 image."""
    r = np.arange(H)[:, None] / max(H, 1)
    c = np.arange(W)[None, :] / max(W, 1)
    base = 0.1 + 0.8 * (0.5 + 0.5 * np.sin(6.0 * r + 1.0)) * (0.5 + 0.5 * np.cos(9.0 * c))
    img = np.stack([np.clip(base * g + rng.normal(0, sigma, (H, W)), 0, 1) for g in (1.0, 0.8, 0.6)], -1)
    return np.rint(img * 255).astype(np.uint8)
