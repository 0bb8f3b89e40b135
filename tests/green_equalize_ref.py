"""NumPy f32 restatement of the green equalisation contract ("Green equalisation"), shared by the green
equalisation tests.  Every intermediate is an np.float32 array and every operation rounds once, in the contract's order.

equalize() is everything the contract defines for every raw pixel from the pre-shading, pre-cast values x; correct() its
y; route_cfa() the work-dtype CFA the route hands to the demosaic (before the defect fix-up); make_frame() the test frames:
column bands that each meet the gate in one way - a flat, noisy field with imbalanced greens (the correction applies), a
field whose imbalance is beyond belief (only |d| <= lim fails), a field where one green phase alternates from quad to quad
(only a range gate fails: the other phase's at the sites of the flat phase, the own phase's at those of the alternating
one), a random two-level texture and a step edge."""
import types

import numpy as np

from oracle import isp_oracle as O

f32 = np.float32
COLOURS = {O.RGGB: (0, 1, 1, 2), O.GRBG: (1, 0, 2, 1), O.GBRG: (1, 2, 0, 1), O.BGGR: (2, 1, 1, 0)}   # of sites 0 .. 3


def green_parity(pattern):
    """gp: (r, c) is green iff ((r + c) & 1) == gp, from the pattern's colour table."""
    return 0 if COLOURS[int(pattern)][0] == 1 else 1


def taps(radius):
    """(the offsets of group O, of group S), each in the contract's order."""
    if radius == 1:
        return [(-1, -1), (-1, 1), (1, -1), (1, 1)], [(0, 0), (-2, 0), (0, -2), (0, 2), (2, 0)]
    odd = [(dy, dx) for dy in (-3, -1, 1, 3) for dx in (-3, -1, 1, 3)]
    even = [(0, 0)] + [(dy, dx) for dy in (-2, 0, 2) for dx in (-2, 0, 2) if (dy, dx) != (0, 0)]
    return odd, even


def _group(xp, H, W, offsets):
    """(sum, n, max, min) over the kept taps of every pixel: the sum in the listed order from the first kept tap."""
    total = np.zeros((H, W), f32)
    n = np.zeros((H, W), np.int32)
    mx = np.full((H, W), -np.inf, f32)
    mn = np.full((H, W), np.inf, f32)
    for dy, dx in offsets:
        q = xp[3 + dy:3 + dy + H, 3 + dx:3 + dx + W]
        kept = np.isfinite(q)
        with np.errstate(invalid="ignore", over="ignore"):
            total = np.where(kept, np.where(n > 0, (total + q).astype(f32), q), total)
        n = n + kept
        mx = np.where(kept, np.maximum(mx, q), mx)
        mn = np.where(kept, np.minimum(mn, q), mn)
    return total, n, mx, mn


def equalize(x, pattern, threshold=1 / 256, slope=1 / 16, strength=1.0, radius=1, edge=4.0, excluded=None):
    """The contract on x (H, W) f32 under the Bayer pattern; excluded: (H, W) bool, the defect map's sites (never a tap; as
    a centre they keep x) or None.  A namespace of (H, W) arrays: y f32; green, apply bool; ok_d, ok_o, ok_s the three gate
    conditions (False wherever nO or nS is 0); n_o, n_s the kept taps; d, lim f32."""
    x = np.asarray(x)
    assert x.dtype == f32 and x.ndim == 2 and radius in (1, 2)
    H, W = x.shape
    t, s, e_f, hs = f32(threshold), f32(slope), f32(edge), f32(f32(strength) * f32(0.5))
    gp = green_parity(pattern)
    listed = np.zeros((H, W), bool) if excluded is None else np.asarray(excluded, bool)
    xp = np.full((H + 6, W + 6), -np.inf, f32)
    xp[3:-3, 3:-3] = np.where(listed, f32(-np.inf), x)
    odd, even = taps(radius)
    sum_o, n_o, max_o, min_o = _group(xp, H, W, odd)
    sum_s, n_s, max_s, min_s = _group(xp, H, W, even)
    r, c = np.mgrid[0:H, 0:W]
    green = ((r + c) & 1) == gp
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mo = (sum_o / n_o.astype(f32)).astype(f32)
        ms = (sum_s / n_s.astype(f32)).astype(f32)
        d = (mo - ms).astype(f32)
        lim = (t + (s * np.maximum(mo, ms)).astype(f32)).astype(f32)
        e = (e_f * lim).astype(f32)
        have = (n_o >= 1) & (n_s >= 1)
        ok_d = have & (np.abs(d) <= lim)
        ok_o = have & ((max_o - min_o).astype(f32) <= e)
        ok_s = have & ((max_s - min_s).astype(f32) <= e)
        apply = green & np.isfinite(x) & ~listed & ok_d & ok_o & ok_s
        y = np.where(apply, (x + (hs * d).astype(f32)).astype(f32), x)
    return types.SimpleNamespace(y=y, green=green, apply=apply, ok_d=ok_d, ok_o=ok_o, ok_s=ok_s, n_o=n_o, n_s=n_s, d=d,
                                 lim=lim)


def _kw(settings, kw):
    if settings is None:
        return kw
    return dict(threshold=settings.threshold, slope=settings.slope, strength=settings.strength, radius=settings.radius,
                edge=settings.edge)


def correct(x, pattern, settings=None, excluded=None, **kw):
    """y (H, W) f32; settings: anything with threshold, slope, strength, radius, edge (a GreenEqualize), or the keywords."""
    return equalize(x, pattern, excluded=excluded, **_kw(settings, kw)).y


def route_cfa(x, pattern, settings, work, gain=None, excluded=None):
    """The route's CFA before the defect fix-up: cast_work(y * g), or cast_work(y) without a grid."""
    y = correct(x, pattern, settings, excluded)
    return O.cast_out(y if gain is None else (y * np.asarray(gain, f32)).astype(f32), work)


# ---- the test frames ---------------------------------------------------------------------------------------------------
def phase_sign(pattern, H, W):
    """+1 at the green sites of even rows, -1 at those of odd rows, 0 elsewhere."""
    r, c = np.mgrid[0:H, 0:W]
    green = ((r + c) & 1) == green_parity(pattern)
    return np.where(green, np.where(r & 1, -1.0, 1.0), 0.0)


def flat_field(rng, H, W, pattern, g=0.25, eps=0.02, sigma=0.005):
    """An f32 field at level g with the greens of even rows at g (1 + eps), those of odd rows at g (1 - eps), and Gaussian
    noise of sigma on every pixel."""
    v = g * (1.0 + eps * phase_sign(pattern, H, W))
    if sigma:
        v = v + rng.normal(0.0, sigma, (H, W))
    return v.astype(f32)


BANDS = (0.40, 0.55, 0.75, 0.90)                         # the right ends of the first four bands, as fractions of W


def make_scene(rng, H, W, pattern):
    """The scene in units of the white level (f64, 0 .. 1): see the module's docstring."""
    r, c = np.mgrid[0:H, 0:W]
    sign = phase_sign(pattern, H, W)
    base = 0.25 + 0.05 * np.sin(3.0 * r / max(H, 1))                       # smooth shading down the rows
    ends = [int(round(f * W)) for f in BANDS]
    v = base * (1.0 + 0.02 * sign)                                         # band 0: +-2 %: applies
    b1 = (c >= ends[0]) & (c < ends[1])
    v = np.where(b1, base * (1.0 + 0.07 * sign), v)                        # band 1: +-7 %: |d| > lim
    b2 = (c >= ends[1]) & (c < ends[2])
    alt = np.where((c >> 1) & 1, -0.05, 0.05)                              # band 2: the odd rows' greens alternate by quad
    v = np.where(b2, base + np.where(sign < 0, alt, 0.0), v)
    v = v + rng.normal(0.0, 0.002, (H, W))
    b3 = (c >= ends[2]) & (c < ends[3])
    v = np.where(b3, np.where(rng.random((H, W)) < 0.5, 0.3, 0.5), v)      # band 3: a two-level texture
    b4 = c >= ends[3]
    v = np.where(b4, np.where(r < H // 2, 0.1, 0.5), v)                    # band 4: a step edge across the rows
    return np.clip(v, 0.0, 1.0)


def make_frame(rng, H, W, pattern, top=4095):
    """(H, W) u16 raw codes in 0 .. top of the scene."""
    return np.rint(make_scene(rng, H, W, pattern) * top).astype(np.uint16)


def coverage(q):
    """From equalize()'s result q, as fractions of the green sites: where the correction applies, and where each gate
    condition is the only one that fails."""
    g = q.green & (q.n_o >= 1) & (q.n_s >= 1)
    n = max(int(q.green.sum()), 1)
    return dict(apply=int(q.apply.sum()) / n,
                only_d=int((g & ~q.ok_d & q.ok_o & q.ok_s).sum()) / n,
                only_o=int((g & q.ok_d & ~q.ok_o & q.ok_s).sum()) / n,
                only_s=int((g & q.ok_d & q.ok_o & ~q.ok_s).sum()) / n)


def assert_exercised(x, pattern, what, excluded=None, **kw):
    """On the reference alone: a frame of 4096 pixels or more has the correction applied on at least 25 % of its green sites
    and each of the three gate conditions the only failing one on at least 1 %."""
    if x.size >= 4096:
        cov = coverage(equalize(x, pattern, excluded=excluded, **kw))
        assert cov["apply"] >= 0.25 and min(cov["only_d"], cov["only_o"], cov["only_s"]) >= 0.01, \
            f"{what}: the frame does not exercise the operator ({cov})"
