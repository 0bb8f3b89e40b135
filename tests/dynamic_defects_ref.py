"""NumPy f32 restatement of the dynamic defects contract ("Dynamic defects"), shared by the dynamic defects
tests.  Every intermediate is an np.float32 array and every operation rounds once, in the contract's order.

detect() is everything the contract defines for every raw pixel from the pre-shading, pre-cast values x; correct() its y;
route_cfa() the work-dtype CFA the route hands to the demosaic (before the defect fix-up); make_frame() the test frames: a
smooth, noisy scene with a sharp edge of each of the four directions, a thin bright line that must stay, and injected hot
and dead pixels - isolated ones of every site, same-site pairs, on the tile seams, on the frame's edges and in its
corners."""
import types

import numpy as np

from oracle import isp_oracle as O

f32 = np.float32
TAPS = [(-2, -2), (-2, 0), (-2, 2), (0, -2), (0, 2), (2, -2), (2, 0), (2, 2)]      # q0 .. q7
PAIRS = [(1, 6), (3, 4), (0, 7), (2, 5)]                 # vertical, horizontal, the two diagonals
GAIN, READ_NOISE = 2.4e-4, 1.5e-3                        # the scene's noise, in units of the white level


def _T(v, t, s):
    """T(v) = t + s max(v, 0): the multiply and the add round once each."""
    return (t + (s * np.maximum(v, f32(0))).astype(f32)).astype(f32)


def detect(x, threshold=0.02, slope=0.2, tolerate=1, hot=True, dead=True, excluded=None):
    """The contract on x (H, W) f32; excluded: (H, W) bool, the defect map's sites (never a tap; as a centre they keep x)
    or None.  A namespace of (H, W) arrays: y f32; hot, dead, flags bool; n the kept taps; hi, lo f32; pair the index of
    the chosen pair (-1: none usable); m its mean; clamped: a replaced pixel whose y is hi / lo although a pair was usable;
    listed_tap: a tap of the pixel is in the map."""
    x = np.asarray(x)
    assert x.dtype == f32 and x.ndim == 2
    assert tolerate in (0, 1) and (hot or dead)
    H, W = x.shape
    t, s, k = f32(threshold), f32(slope), int(tolerate)
    listed = np.zeros((H, W), bool) if excluded is None else np.asarray(excluded, bool)
    xp = np.full((H + 4, W + 4), -np.inf, f32)
    xp[2:-2, 2:-2] = np.where(listed, f32(-np.inf), x)
    lp = np.zeros((H + 4, W + 4), bool)
    lp[2:-2, 2:-2] = listed
    Q = np.stack([xp[2 + dr:2 + dr + H, 2 + dc:2 + dc + W] for dr, dc in TAPS])
    kept = np.isfinite(Q)
    n = kept.sum(axis=0)
    hi = np.sort(np.where(kept, Q, f32(-np.inf)), axis=0)[7 - k]
    lo = np.sort(np.where(kept, Q, f32(np.inf)), axis=0)[k]
    cand = (n >= 2 * k + 1) & np.isfinite(x) & ~listed
    with np.errstate(invalid="ignore", over="ignore"):
        is_hot = cand & bool(hot) & ((x - hi).astype(f32) > _T(hi, t, s))
        is_dead = cand & bool(dead) & ((lo - x).astype(f32) > _T(lo, t, s))
        assert not (is_hot & is_dead).any()
        have = np.zeros((H, W), bool)
        best = np.zeros((H, W), f32)
        m = np.zeros((H, W), f32)
        which = np.full((H, W), -1)
        for i, (a, b) in enumerate(PAIRS):
            usable = kept[a] & kept[b]
            d = np.abs((Q[a] - Q[b]).astype(f32))
            take = usable & (~have | (d < best))
            best = np.where(take, d, best)
            m = np.where(take, ((Q[a] + Q[b]).astype(f32) * f32(0.5)).astype(f32), m)
            which = np.where(take, i, which)
            have |= usable
        y_hot = np.where(have, np.minimum(m, hi), hi)
        y_dead = np.where(have, np.maximum(m, lo), lo)
    y = np.where(is_hot, y_hot, np.where(is_dead, y_dead, x)).astype(f32)
    flags = is_hot | is_dead
    clamped = have & ((is_hot & (m > hi)) | (is_dead & (m < lo)))
    listed_tap = np.stack([lp[2 + dr:2 + dr + H, 2 + dc:2 + dc + W] for dr, dc in TAPS]).any(axis=0)
    return types.SimpleNamespace(y=y, hot=is_hot, dead=is_dead, flags=flags, n=n, hi=hi, lo=lo, pair=np.where(flags, which, -2),
                                 m=m, clamped=clamped, listed_tap=listed_tap)


def correct(x, settings=None, excluded=None, **kw):
    """y (H, W) f32; settings: anything with threshold, slope, tolerate, hot, dead (a DynamicDefects), or the keywords."""
    return detect(x, excluded=excluded, **_kw(settings, kw)).y


def _kw(settings, kw):
    if settings is None:
        return kw
    return dict(threshold=settings.threshold, slope=settings.slope, tolerate=settings.tolerate, hot=settings.hot,
                dead=settings.dead)


def route_cfa(x, settings, work, gain=None, excluded=None):
    """The route's CFA before the defect fix-up: cast_work(y * g), or cast_work(y) without a grid."""
    y = correct(x, settings, excluded)
    return O.cast_out(y if gain is None else (y * np.asarray(gain, f32)).astype(f32), work)


def mask_words(flags):
    """The flag plane of a boolean (H, W) mask: DefectMap.mask_words()' layout, for any size."""
    H, W = flags.shape
    mw = (W + 31) // 32
    bits = np.zeros((H, mw * 32), bool)
    bits[:, :W] = flags
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(H, mw)


# ---- the test frames ---------------------------------------------------------------------------------------------------
def _scene(rng, H, W):
    """The defect-free scene in units of the white level: smooth shading in 0.15 .. 0.45; four 20 x 20 patches, each a
    sharp step of 0.15 through its centre (horizontal, vertical and the two diagonal edges) under a raised-cosine window,
    so the step fades out along its edge instead of ending in a tip; a one-pixel vertical line up to 0.2 brighter, faded out
    toward the frame's top and bottom (a line that ended, or met the frame's edge, at full height would be a defect to any
    detector of this kind); shot and read noise on top."""
    r = np.arange(H)[:, None].astype(np.float64)
    c = np.arange(W)[None, :].astype(np.float64)
    v = 0.15 + 0.3 * (0.5 + 0.5 * np.sin(5.0 * r / max(H, 1) + 1.0)) * (0.5 + 0.5 * np.cos(7.0 * c / max(W, 1)))
    for (rc, cc), side in zip(PATCHES, (lambda dr, dc: dr >= 0, lambda dr, dc: dc >= 0,
                                        lambda dr, dc: dr - dc >= 0, lambda dr, dc: dr + dc >= 0)):
        dr, dc = r - rc, c - cc
        win = np.where((np.abs(dr) < 10) & (np.abs(dc) < 10),
                       (0.5 + 0.5 * np.cos(np.pi * dr / 10)) * (0.5 + 0.5 * np.cos(np.pi * dc / 10)), 0.0)
        v = v + 0.15 * win * side(dr, dc)
    if H >= 32 and W > LINE_COL + 2:
        v[:, LINE_COL] += 0.2 * np.sin(np.pi * (np.arange(H) + 0.5) / H) ** 2
    sigma = np.sqrt(GAIN * v + READ_NOISE ** 2)
    return np.clip(v + rng.normal(0.0, 1.0, (H, W)) * sigma, 0.0, 1.0)


PATCHES = [(14, 14), (14, 40), (40, 14), (40, 40)]       # the centres of the four edge patches: each holds a hot pixel
LINE_COL = 58


def injections(H, W):
    """(hot sites, dead sites, pair members, sites a DefectMap of the frame should list) of an H x W frame: what fits."""
    hot = list(PATCHES)                                                   # on each edge: each pair is chosen somewhere
    hot += [(28, 6), (28, 13), (29, 20), (29, 27)]                        # isolated, one per site
    dead = [(28, 34), (28, 41), (29, 48), (29, 55)]
    pairs = [(52, 6), (52, 8), (52, 16), (54, 18)]                        # distance 2 along a row, along a diagonal
    pairs += [(0, 30), (0, 32)]                                           # on the frame's top edge: one usable pair, the clamp
    hot += [(0, 0), (H - 1, 0), (63, 26), (64, 33), (20, 63), (21, 64), (63, 63), (64, 64)]    # corners, seams
    dead += [(H - 1, W - 1), (34, 0), (0, W - 1), (63, 44), (64, 51), (46, 63), (47, 64)]
    listed = [(28, 8), (26, 34), (52, 4), (1, 1), (63, 64), (H - 2, W - 2)]   # next to dynamic ones, and elsewhere
    inside = lambda sites: [(a, b) for a, b in sites if 0 <= a < H and 0 <= b < W]
    hot, dead, pairs, listed = inside(hot), inside(dead), inside(pairs), inside(listed)
    taken, out = set(), []
    for group in (pairs, hot, dead):                                      # no defect in another one's taps, but the pairs
        kept = []
        for a, b in group:
            near = any((a + dr, b + dc) in taken for dr in (-2, 0, 2) for dc in (-2, 0, 2))
            if group is pairs or not near:
                kept.append((a, b))
                taken.add((a, b))
        out.append(kept)
    pairs, hot, dead = out
    listed = [p for p in listed if p not in taken]
    return hot, dead, pairs, listed


def make_frame(rng, H, W, top=4095, inject=True):
    """((H, W) u16 raw codes in 0 .. top of the scene, info).  inject: hot pixels (the scene plus half the range) and dead
    ones (code 0) at injections(H, W).  info: a namespace of hot, dead, pairs (both members hot) and listed, lists of
    (row, col); listed is for the caller's DefectMap and is not touched here."""
    v = _scene(rng, H, W)
    hot, dead, pairs, listed = injections(H, W)
    if inject:
        for a, b in hot + pairs:
            v[a, b] = min(v[a, b] + 0.5, 1.0)
        for a, b in dead:
            v[a, b] = 0.0
    codes = np.rint(v * top).astype(np.uint16)
    return codes, types.SimpleNamespace(hot=hot, dead=dead, pairs=pairs, listed=listed)


def listed_mask(info, H, W):
    m = np.zeros((H, W), bool)
    for a, b in info.listed:
        m[a, b] = True
    return m


def coverage(d, excluded=None):
    """What a frame of 4096 pixels or more must show, from detect()'s result d: a dict of counts, each of which must be
    positive (listed_tap only with a map)."""
    out = dict(hot=int(d.hot.sum()), dead=int(d.dead.sum()), fallback=int((d.pair == -1).sum()),
               clamped=int(d.clamped.sum()))
    for i in range(4):
        out[f"pair{i}"] = int((d.pair == i).sum())
    if excluded is not None:
        out["listed_tap"] = int((d.flags & d.listed_tap).sum())
    return out


def assert_exercised(x, what, threshold=0.02, excluded=None):
    """On the reference alone, at the default settings (threshold in the units of x): a frame of 4096 pixels or more shows
    hot and dead pixels, each of the four pairs chosen, the no-usable-pair fallback, the clamp active and, with a map, a
    flagged pixel with a listed tap."""
    if x.size >= 4096:
        cov = coverage(detect(x, threshold=threshold, excluded=excluded), excluded)
        assert min(cov.values()) > 0, f"{what}: the frame does not exercise the operator ({cov})"
