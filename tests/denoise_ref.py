"""NumPy f64 restatement of the raw noise reduction contract ("Raw noise reduction"), shared by the denoise
tests.

filter_x() is y of every raw pixel from the pre-shading, pre-cast values x (f64 throughout, the settings rounded to f32
as the C ABI takes them); assert_within_bound() is the stated bound of the work-dtype CFA: within one unit in the last
place of the work dtype of round(y * g), and for f32 also within 1e-5 of y * g relative or within the smallest normal f32
absolute (the hardware exp and rcp flush f32 subnormals: a y * g below 2^-126 may come out as 0)."""
import numpy as np

f32 = np.float32


def settings(dn):
    """(gain, read_noise, strength, spatial_sigma, radius) as the kernel gets them (f32 values, widened)."""
    return (float(f32(dn.gain)), float(f32(dn.read_noise)), float(f32(dn.strength)), float(f32(dn.spatial_sigma)),
            int(dn.radius))


def filter_x(x, dn, excluded=None, step=2):
    """y (H, W) f64: x (H, W) any float array, excluded (H, W) bool (the defect map's sites: never a neighbour) or None.
    step: the distance between taps in raw pixels (2: same-site; the contract has no other)."""
    gain, rn, st, sg, R = settings(dn)
    x = np.asarray(x, np.float64)
    H, W = x.shape
    ok = np.ones((H, W), bool) if excluded is None else ~np.asarray(excluded, bool)
    P = step * R
    xp = np.zeros((H + 2 * P, W + 2 * P))
    vp = np.zeros((H + 2 * P, W + 2 * P), bool)
    xp[P:P + H, P:P + W] = x
    vp[P:P + H, P:P + W] = ok
    var = gain * np.maximum(x, 0.0) + rn * rn
    k = 1.0 / (2.0 * st * st * var)
    num = x.copy()
    den = np.ones_like(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(-R, R + 1):
            for j in range(-R, R + 1):
                if i == 0 and j == 0:
                    continue
                q = xp[P + step * i:P + step * i + H, P + step * j:P + step * j + W]
                v = vp[P + step * i:P + step * i + H, P + step * j:P + step * j + W]
                w = np.where(v, np.exp(-(q - x) ** 2 * k - (i * i + j * j) / (2.0 * sg * sg)), 0.0)
                num += w * np.where(v, q, 0.0)
                den += w
    return num / den


def route_yg(x, dn, gain=None, excluded=None):
    """y * g (f64) of the route's CFA before the cast and the defect fix-up; gain (H, W) f32 or None."""
    y = filter_x(x, dn, excluded)
    return y if gain is None else y * np.asarray(gain, np.float64)


def assert_within_bound(got, yg, work, what="", where=None):
    """got: the work-dtype CFA; yg: the f64 y * g of the contract; where: (H, W) bool of the pixels to check (None: all)."""
    dt = np.float16 if work == "f16" else np.float32
    ref = np.asarray(yg, np.float64).astype(dt)
    g = np.asarray(got).astype(dt).astype(np.float64)
    diff = np.abs(g - ref.astype(np.float64))
    ok = diff <= np.spacing(np.abs(ref)).astype(np.float64)
    if work == "f32":
        ok |= diff <= 1e-5 * np.abs(np.asarray(yg, np.float64))
        ok |= diff < float(np.finfo(np.float32).tiny)
    if where is not None:
        ok |= ~np.asarray(where, bool)
    if not ok.all():
        r, c = np.argwhere(~ok)[0]
        raise AssertionError(f"{what}: {(~ok).sum()} pixels outside the bound; first ({r}, {c}): got {g[r, c]!r}, "
                             f"f64 {float(yg[r, c])!r} (rounded {float(ref[r, c])!r})")
