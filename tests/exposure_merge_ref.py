"""NumPy f32 restatement of the exposure merge contract ("Exposure merge"), shared by the exposure merge
tests.  Every intermediate is an np.float32 array and every operation rounds once (one .astype(float32) each), in the
contract's order.

merge() is the stage's y from the pre-shading, pre-cast values x_e of a bracket (the shortest exposure first); detail() the
per-frame u, k, w and the tap count; classes() the fractions of a bracket in the four classes the tests need;
make_bracket() a bracket that puts every class in a frame; static_bracket() a bracket drawn from the noise model;
rounding_bracket() one whose y follows every rounding."""
import numpy as np

f32 = np.float32


class Settings:
    """The settings as the library rounds them.  mi_isp_exposure_merge holds them as f32; from those values the library
    computes inv_e = 1 / ratio_e, i2_e = 1 / ratio_e^2, rn2 = read_noise^2, c = threshold^2, rf = 1 / (saturation * knee)
    and R[n] = 1 / n in double and rounds each once."""

    def __init__(self, ratios, gain, read_noise, saturation=0.9, knee=0.25, threshold=4.0):
        r = [float(f32(q)) for q in ratios]
        self.E = len(r)
        self.ratios = r
        self.inv = [f32(1.0 / q) for q in r]
        self.i2 = [f32(1.0 / (q * q)) for q in r]
        self.gain = f32(gain)
        self.rn2 = f32(float(f32(read_noise)) * float(f32(read_noise)))
        self.c = f32(float(f32(threshold)) * float(f32(threshold)))
        self.sat = f32(saturation)
        self.knee = f32(knee)
        self.rf = f32(1.0 / (float(f32(saturation)) * float(f32(knee))))
        self.R = np.array([0.0] + [1.0 / n for n in range(1, 10)], np.float64).astype(f32)


def as_settings(s):
    """A Settings from a Settings, a (ratios, gain, read_noise[, saturation[, knee[, threshold]]]) tuple or an
    ExposureMerge."""
    if isinstance(s, Settings):
        return s
    if isinstance(s, (tuple, list)):
        return Settings(*s)
    return Settings(s.ratios, s.gain, s.read_noise, s.saturation, s.knee, s.threshold)


TAPS = [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)]    # the contract's order


def metric(x0, se, kept, R, taps=TAPS):
    """(m, n): the mean absolute difference of se to x0 over every pixel's kept taps, and the number of those."""
    H, W = x0.shape
    d = np.abs((se - x0).astype(f32)).astype(f32)
    dp = np.zeros((H + 4, W + 4), f32)
    kp = np.zeros((H + 4, W + 4), bool)
    dp[2:-2, 2:-2] = d
    kp[2:-2, 2:-2] = kept
    D = np.zeros((H, W), f32)
    n = np.zeros((H, W), np.int64)
    for i, j in taps:
        dq = dp[2 + 2 * i:2 + 2 * i + H, 2 + 2 * j:2 + 2 * j + W]
        kq = kp[2 + 2 * i:2 + 2 * i + H, 2 + 2 * j:2 + 2 * j + W]
        D = np.where(kq, np.where(n > 0, (D + dq).astype(f32), dq), D).astype(f32)       # from its first kept term
        n = n + kq
    return (D * R[n]).astype(f32), n


def detail(frames, settings, excluded=None, taps=TAPS):
    """(n, [(u, k, w) of every long frame]) of a bracket: frames E (H, W) f32 arrays, the shortest exposure first;
    excluded: (H, W) bool, the defect map's sites (never a tap), or None.  taps: the order of the sum (the contract's; a
    test passes another one to show that its bracket tells the orders apart)."""
    s = as_settings(settings)
    frames = [np.asarray(x) for x in frames]
    assert len(frames) == s.E and all(x.dtype == f32 and x.ndim == 2 and x.shape == frames[0].shape for x in frames)
    x0 = frames[0]
    kept = np.ones(x0.shape, bool) if excluded is None else ~np.asarray(excluded, bool)
    v0 = ((s.gain * np.maximum(x0, f32(0))).astype(f32) + s.rn2).astype(f32)
    out = []
    n = np.zeros(x0.shape, np.int64)
    for e in range(1, s.E):
        xe = frames[e]
        se = (xe * s.inv[e]).astype(f32)
        m, n = metric(x0, se, kept, s.R, taps)
        ve = (((s.gain * np.maximum(xe, f32(0))).astype(f32) + s.rn2).astype(f32) * s.i2[e]).astype(f32)
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            qv = ((m * m).astype(f32) / (s.c * (v0 + ve).astype(f32)).astype(f32)).astype(f32)
            k = np.maximum((f32(1) - qv).astype(f32), f32(0)).astype(f32)
            u = np.minimum(np.maximum(((s.sat - xe).astype(f32) * s.rf).astype(f32), f32(0)), f32(1)).astype(f32)
            w = ((u * k).astype(f32) / ve).astype(f32)
        out.append((u, k, w))
    if s.E == 1:
        _, n = metric(x0, x0, kept, s.R, taps)
    return n, out


def merge(frames, settings, excluded=None, taps=TAPS, order=None):
    """y (H, W) f32.  order: the order in which the long frames enter num and den (the contract's 1 .. E - 1; a test passes
    the reversed one to show that its bracket tells the orders apart)."""
    s = as_settings(settings)
    n, per = detail(frames, s, excluded, taps)
    x0 = np.asarray(frames[0])
    v0 = ((s.gain * np.maximum(x0, f32(0))).astype(f32) + s.rn2).astype(f32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        a0 = (f32(1) / v0).astype(f32)
        num = (a0 * x0).astype(f32)
        den = a0
        used = np.zeros(x0.shape, bool)
        for e in (range(1, s.E) if order is None else order):
            _, _, w = per[e - 1]
            se = (np.asarray(frames[e]) * s.inv[e]).astype(f32)
            take = w > 0
            num = np.where(take, (num + (w * se).astype(f32)).astype(f32), num).astype(f32)
            den = np.where(take, (den + w).astype(f32), den).astype(f32)
            used |= take
        y = (num / den).astype(f32)
    return np.where((n == 0) | ~used, x0, y).astype(f32)


def classes(frames, settings, excluded=None):
    """The fractions of the pixels in the four classes a test bracket must show, from the reference alone: (shortest only
    because every long frame is saturated (u == 0 everywhere), shortest only because the usable long frames were rejected
    (no frame used, some frame with u > 0), some used long frame inside its knee (0 < u < 1, w > 0), every long frame
    fully usable (u == 1 and k > 0 for all))."""
    n, per = detail(frames, settings, excluded)
    us = np.stack([u for u, _, _ in per])
    ks = np.stack([k for _, k, _ in per])
    ws = np.stack([w for _, _, w in per])
    used = (ws > 0).any(0) & (n > 0)
    saturated = (us == 0).all(0)
    rejected = ~used & (us > 0).any(0)
    knee = ((us > 0) & (us < 1) & (ws > 0)).any(0) & (n > 0)
    full = ((us == 1) & (ks > 0)).all(0) & (n > 0)
    return float(saturated.mean()), float(rejected.mean()), float(knee.mean()), float(full.mean())


def noise_sigma(clean, gain, read_noise):
    """The model's standard deviation at the clean values, f64."""
    return np.sqrt(float(gain) * np.maximum(np.asarray(clean, np.float64), 0) + float(read_noise) ** 2)


def expose(rng, radiance, ratio, gain, read_noise, top=1.0):
    """One exposure of the scene `radiance` (in the units of the shortest frame, f64) at `ratio`: the scaled scene plus
    noise drawn from the model at that level, clipped to [0, top] as a sensor does."""
    clean = np.asarray(radiance, np.float64) * float(ratio)
    return np.clip(clean + rng.normal(0, 1, clean.shape) * noise_sigma(clean, gain, read_noise), 0.0, top)


BLOCK = 16                                                  # make_bracket's class blocks (pixels)


def make_bracket(rng, H, W, ratios, gain, read_noise, saturation=0.9, knee=0.25):
    """E frames of values in [0, 1] (f64), the shortest exposure first, for the kernel tests.  The scene is made of
    16 x 16 blocks placed for the ratios and the knee, five kinds in a pattern that puts every kind next to every tile
    seam: dark enough for every long frame to be fully usable; inside the knee of the first long frame; bright enough
    to saturate every long frame; dark in the shortest frame and something else (mid-grey) in the long ones - a moved
    object, which must be rejected; and a log ramp over the whole range."""
    ratios = [float(q) for q in ratios]
    r1, rmax = ratios[1], ratios[-1]
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    kind = ((rr // BLOCK) + 2 * (cc // BLOCK)) % 5
    t = rng.random((H, W))
    dark = saturation * (1 - knee) / rmax * (0.15 + 0.6 * t)
    in_knee = saturation / r1 * (1 - knee * (0.1 + 0.8 * t))
    bright = np.minimum(saturation / r1 * (1.1 + 2.0 * t), 0.97)
    ramp = 0.9 * np.exp(np.log(saturation / rmax * 0.05 / 0.9) * (1 - (rr * W + cc) / max(H * W - 1, 1)))
    scene = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [dark, in_knee, bright, dark], ramp)
    moved = np.where(kind == 3, saturation / r1 * (0.35 + 0.3 * t), scene)              # what the long frames see
    return [expose(rng, scene if e == 0 else moved, q, gain, read_noise) for e, q in enumerate(ratios)]


def smooth_scene(H, W, lo=0.002, hi=0.8):
    """A smooth clean scene over the whole range [lo, hi] (log-spaced along a wave), f64."""
    r = np.arange(H)[:, None] / max(H, 1)
    c = np.arange(W)[None, :] / max(W, 1)
    t = (0.5 + 0.5 * np.sin(3.0 * r + 0.5)) * (0.5 + 0.5 * np.cos(4.0 * c))
    return lo * np.exp(np.log(hi / lo) * t)


def static_bracket(rng, scene, ratios, gain, read_noise):
    """A bracket of the static `scene` drawn from the noise model, f32 frames (no quantisation)."""
    return [expose(rng, scene, q, gain, read_noise).astype(f32) for q in ratios]


def rounding_bracket(rng, H, W):
    """(frames, (ratios, gain, read_noise, saturation, knee, threshold)): three frames whose differences, against a low
    threshold, keep almost every
    k partial, with many pixels inside a wide knee, so that y follows every rounding of D, m, qv, k, u and w (the tap order
    and the order of the exposures included)."""
    ratios = (1.0, 2.0, 4.0)
    x0 = (0.01 + 0.25 * rng.random((H, W))).astype(f32)
    frames = [x0]
    for q in ratios[1:]:
        frames.append(np.clip((x0 + rng.uniform(-0.05, 0.05, (H, W))) * q, 0, 1).astype(f32))
    return frames, (ratios, 0.01, 0.05, 0.9, 0.5, 0.5)
