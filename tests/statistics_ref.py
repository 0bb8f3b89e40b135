"""NumPy restatement of the frame statistics contract ("Frame statistics"), shared by the statistics tests.
Written from the definitions, pixel sets and integer sums only: nothing here knows of tiles, lanes or launches.

measure() is everything the contract defines for one frame from the pre-shading, pre-cast values x: a namespace of the
int64 arrays zones (gh, gw, 4, 4), focus (gh, gw, 2), histogram (4, 256), words (their concatenation, the device buffer's
layout) and the per-pixel intermediates the tests reason about.  make_scene() is the GPU tests' generated input and
assert_exercised() the conditions it has to meet, checked on the reference alone."""
import types

import numpy as np

from oracle import isp_oracle as O

f32 = np.float32
COLOURS = {O.RGGB: (0, 1, 1, 2), O.GRBG: (1, 0, 2, 1), O.GBRG: (1, 2, 0, 1), O.BGGR: (2, 1, 1, 0)}   # of sites 0 .. 3
TAPS = ((-2, 0), (2, 0), (0, -2), (0, 2))
BINS = 256


def green_parity(pattern):
    """gp: (r, c) is green iff ((r + c) & 1) == gp, from the pattern's colour table."""
    return 0 if COLOURS[int(pattern)][0] == 1 else 1


def words(zones):
    return zones[0] * zones[1] * 18 + 4 * BINS


def _sum_by(index, values, n):
    """The int64 sums of the non-negative int64 values (None: ones) per index 0 .. n - 1, exact: np.bincount adds in f64, so
    the values go in as two halves of 20 and at most 17 bits, whose sums over 2^26 pixels stay below 2^53."""
    if values is None:
        return np.bincount(index, minlength=n).astype(np.int64)
    lo = np.bincount(index, weights=(values & 0xFFFFF).astype(np.float64), minlength=n).astype(np.int64)
    hi = np.bincount(index, weights=(values >> 20).astype(np.float64), minlength=n).astype(np.int64)
    return (hi << 20) + lo


def measure(x, pattern, zones=(8, 8), clip=0.98, dark=1 / 64, excluded=None):
    """The contract on x (H, W) f32, H and W even, under the Bayer pattern; excluded: (H, W) bool, the defect map's sites,
    or None."""
    x = np.asarray(x)
    assert x.dtype == f32 and x.ndim == 2
    H, W = x.shape
    gh, gw = zones
    assert H % 2 == 0 and W % 2 == 0 and 1 <= gh <= H // 2 and 1 <= gw <= W // 2 and H * W <= 1 << 26
    t, d = f32(clip), f32(dark)
    listed = np.zeros((H, W), bool) if excluded is None else np.asarray(excluded, bool)
    with np.errstate(invalid="ignore"):
        valid = ~listed & (x > f32(-np.inf))                                  # (a NaN compares false)
        u = np.minimum(np.maximum(np.where(valid, x, f32(0)), f32(0)), f32(1))
        v = np.rint((u * f32(65536)).astype(f32)).astype(np.int64)            # (np.rint: ties to even)
        clipped = valid & (x >= t)
        is_dark = valid & (x <= d)
        below = valid & (x < t)
    v = np.where(valid, v, 0)
    r, c = np.mgrid[0:H, 0:W]
    site = (r & 1) * 2 + (c & 1)
    zi = ((r >> 1) * gh) // (H // 2)
    zj = ((c >> 1) * gw) // (W // 2)
    cell = zi * gw + zj
    Z = np.stack([_sum_by((cell * 4 + site).ravel(), q.ravel(), gh * gw * 4)
                  for q in (valid.astype(np.int64), v, clipped.astype(np.int64), is_dark.astype(np.int64))],
                 axis=-1).reshape(gh, gw, 4, 4)
    hist = _sum_by(site[valid] * BINS + np.minimum(v[valid] >> 8, BINS - 1), None, 4 * BINS).reshape(4, BINS)
    # focus: the green pixels whose four same-site taps are valid, centre and taps below clip
    green = ((r + c) & 1) == green_parity(pattern)
    bp = np.zeros((H + 4, W + 4), bool)
    bp[2:-2, 2:-2] = below
    vp = np.zeros((H + 4, W + 4), np.int64)
    vp[2:-2, 2:-2] = v
    vl = np.zeros((H + 4, W + 4), bool)
    vl[2:-2, 2:-2] = valid
    taps_valid = np.ones((H, W), bool)
    taps_below = np.ones((H, W), bool)
    total = np.zeros((H, W), np.int64)
    for dy, dx in TAPS:
        taps_valid &= vl[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
        taps_below &= bp[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
        total += vp[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
    candidate = green & valid & taps_valid                                     # everything but the clip rule
    contributes = candidate & below & taps_below
    L = np.where(contributes, 4 * v - total, 0)
    F = np.stack([_sum_by(cell.ravel(), (L * L).ravel(), gh * gw),
                  _sum_by(cell.ravel(), contributes.astype(np.int64).ravel(), gh * gw)], axis=-1).reshape(gh, gw, 2)
    return types.SimpleNamespace(zones=Z, focus=F, histogram=hist,
                                 words=np.concatenate([Z.ravel(), F.ravel(), hist.ravel()]), valid=valid, v=v,
                                 clipped=clipped, dark=is_dark, green=green, candidate=candidate, contributes=contributes,
                                 tap_rejected=candidate & below & ~taps_below,
                                 L=L, zi=zi, zj=zj, site=site)


def of(settings, x, pattern, excluded=None):
    """measure() under a Statistics (anything with zones, clip, dark)."""
    return measure(x, pattern, tuple(settings.zones), settings.clip, settings.dark, excluded)


# ---- the helpers of FrameStatistics, as the same f64 expressions on the reference's integers --------------------------------
def _ratio(Z, k):
    z = Z.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(z[..., 0] > 0, z[..., k] / z[..., 0], np.nan)


def mean(q):
    return _ratio(q.zones, 1) / 65536.0


def clipped_fraction(q):
    return _ratio(q.zones, 2)


def dark_fraction(q):
    return _ratio(q.zones, 3)


def sharpness(q):
    f = q.focus.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(f[..., 1] > 0, f[..., 0] / f[..., 1] / 2.0 ** 32, np.nan)


def percentile(q, p, site=None):
    h = q.histogram.sum(axis=0) if site is None else q.histogram[site]
    total = int(h.sum())
    if total == 0:
        return float("nan")
    k = int(np.searchsorted(np.cumsum(h).astype(np.float64), p / 100.0 * total, side="left"))
    return min(k, BINS - 1) / float(BINS)


# ---- the test frames ---------------------------------------------------------------------------------------------------
def make_scene(rng, H, W):
    """The scene in units of the white level (f64, 0 .. 1): a smooth ramp over the whole range with fine texture, blown
    out blobs (plateaus at 1.0, about a quarter of the frame, with the rims that the focus rule rejects) and black blobs (a
    fifth)."""
    r, c = np.mgrid[0:H, 0:W]
    ramp = 0.04 + 0.9 * ((r * 0.37 + c * 0.63) % 1.0 * 0.15 + 0.85 * (r / max(H - 1, 1) * 0.5 + c / max(W - 1, 1) * 0.5))
    v = ramp + rng.normal(0.0, 0.02, (H, W))
    cell = max(4, min(H, W) // 12)
    blob = rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell))
    up = np.kron(blob, np.ones((cell, cell)))[:H, :W]
    v = np.where(up < 0.25, 1.0, v)
    v = np.where(up > 0.80, rng.random((H, W)) * 0.01, v)
    return np.clip(v, 0.0, 1.0)


def make_frame(rng, H, W, top=4095):
    """(H, W) u16 raw codes in 0 .. top of the scene."""
    return np.rint(make_scene(rng, H, W) * top).astype(np.uint16)


def coverage(q):
    n = max(int(q.valid.sum()), 1)
    g = max(int((q.green & q.valid).sum()), 1)
    return dict(clipped=int(q.clipped.sum()) / n, dark=int(q.dark.sum()) / n,
                focus=int(q.contributes.sum()) / g, rejected=int(q.tap_rejected.sum()) / g,
                bins=int((q.histogram > 0).sum(axis=1).min()), empty_zones=int((q.zones[..., 0].sum(axis=2) == 0).sum()))


def assert_exercised(q, what, normalised=True):
    """On the reference alone, for a generated frame of 4096 pixels or more: 5 .. 50 % of the pixels clipped, at least 5 %
    dark, at least 25 % of the green pixels contributing to F and at least 5 % of them rejected for a clipped tap (the
    centre itself below clip), at least 64 histogram bins occupied per site, every zone non-empty.  normalised=False: x
    is in codes (load_16f), where every v but that of code 0 is 65536 - the bins are two by definition."""
    cov = coverage(q)
    assert cov["empty_zones"] == 0, f"{what}: an empty zone ({cov})"
    if q.valid.size >= 4096:
        assert 0.05 <= cov["clipped"] <= 0.5 and cov["dark"] >= 0.05 and cov["focus"] >= 0.25 \
            and cov["rejected"] >= 0.05 and (cov["bins"] >= 64 or not normalised), f"{what}: the frame does not exercise the statistics ({cov})"
