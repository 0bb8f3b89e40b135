"""NumPy f32 restatement of the temporal noise reduction contract ("Temporal noise reduction"), shared by the
temporal tests.  Every intermediate is an np.float32 array and every operation rounds once (one .astype(float32) each), in
the contract's order.

weights() is (w, n) of every raw pixel, blend() the filter's y (= the next history) from the pre-shading, pre-cast values
x and the history h; coverage() the fractions of a frame in the three weight classes the tests need; noisy() draws a frame
from the noise model."""
import numpy as np

f32 = np.float32


class Settings:
    """The four settings as the library rounds them.  mi_isp_temporal holds them as f32; from those values the library
    computes rn2 = read_noise^2, c = threshold^2 and R[n] = 1 / n in double and rounds each once."""

    def __init__(self, gain, read_noise, threshold=3.0, max_weight=0.75):
        self.gain = f32(gain)
        self.rn2 = f32(float(f32(read_noise)) * float(f32(read_noise)))
        self.c = f32(float(f32(threshold)) * float(f32(threshold)))
        self.wmax = f32(max_weight)
        self.R = np.array([0.0] + [1.0 / n for n in range(1, 10)], np.float64).astype(f32)


def as_settings(s):
    """A Settings from a Settings, a (gain, read_noise[, threshold[, max_weight]]) tuple or a TemporalDenoise."""
    if isinstance(s, Settings):
        return s
    if isinstance(s, (tuple, list)):
        return Settings(*s)
    return Settings(s.gain, s.read_noise, s.threshold, s.max_weight)


TAPS = [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)]    # the contract's order


def weights(x, h, settings, excluded=None, taps=TAPS):
    """(w, n): the weight of the past (H, W) f32 and the number of kept taps (H, W) int of every pixel.  x, h: (H, W) f32;
    excluded: (H, W) bool, the defect map's sites (never a tap), or None.  taps: the order of the sum (the contract's; a
    test passes another one to show that its frame tells the orders apart)."""
    s = as_settings(settings)
    x, h = np.asarray(x), np.asarray(h)
    assert x.dtype == f32 and h.dtype == f32 and x.shape == h.shape and x.ndim == 2
    H, W = x.shape
    kept = np.ones((H, W), bool) if excluded is None else ~np.asarray(excluded, bool)
    d = np.abs((x - h).astype(f32)).astype(f32)
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
    m = (D * s.R[n]).astype(f32)
    var = ((s.gain * np.maximum(h, f32(0))).astype(f32) + s.rn2).astype(f32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        qv = ((m * m).astype(f32) / (s.c * var).astype(f32)).astype(f32)
    k = np.maximum((f32(1) - qv).astype(f32), f32(0)).astype(f32)
    w = (s.wmax * k).astype(f32)
    return w, n


def blend(x, h, settings, excluded=None, taps=TAPS):
    """y (H, W) f32 = the history after the frame.  h None: an empty history, y = x."""
    x = np.asarray(x)
    assert x.dtype == f32 and x.ndim == 2
    if h is None:
        return x.copy()
    w, n = weights(x, h, settings, excluded, taps)
    y = (x + (w * (h - x).astype(f32)).astype(f32)).astype(f32)
    return np.where((n == 0) | (w == 0), x, y).astype(f32)


def run(frames, settings, excluded=None, h=None):
    """The ys of a sequence of frames through one history (h: the history before the first, None for empty)."""
    out = []
    for x in frames:
        h = blend(x, h, settings, excluded)
        out.append(h)
    return out


def coverage(x, h, settings, excluded=None):
    """(the fractions of the pixels with w == 0, 0 < w <= wmax / 2 and w > wmax / 2, every pixel with w > 0 and h != x
    changes): what a test frame must show for the operator to be exercised, from the reference alone."""
    s = as_settings(settings)
    w, n = weights(x, h, s, excluded)
    w = np.where(n == 0, f32(0), w)
    half = f32(float(s.wmax) / 2)
    y = blend(x, h, s, excluded)
    moved = (w > 0) & (h != x)
    return (float((w == 0).mean()), float(((w > 0) & (w <= half)).mean()), float((w > half).mean()),
            bool(np.all(y[moved] != x[moved])))


def noise_sigma(clean, gain, read_noise):
    """The model's standard deviation at the clean values, f64."""
    return np.sqrt(float(gain) * np.maximum(np.asarray(clean, np.float64), 0) + float(read_noise) ** 2)


def noisy(rng, clean, gain, read_noise):
    """A frame drawn from the noise model around `clean`, f32."""
    return (np.asarray(clean, np.float64) + rng.normal(0, 1, np.shape(clean)) * noise_sigma(clean, gain, read_noise)).astype(f32)


def smooth_scene(H, W):
    """A smooth clean scene in [0.15, 0.75], f64."""
    r = np.arange(H)[:, None] / max(H, 1)
    c = np.arange(W)[None, :] / max(W, 1)
    return 0.15 + 0.6 * (0.5 + 0.5 * np.sin(3.0 * r + 0.5)) * (0.5 + 0.5 * np.cos(4.0 * c))


def next_frame(rng, prev, gain, read_noise):
    """The frame after `prev` (values in [0, 1], f64) for the kernel tests: prev plus fresh model noise; the top left
    quarter replaced by random values (motion: the past must be dropped) and the bottom right quarter offset by 2.4 noise
    standard deviations (the partial weights).  Clipped to [0.02, 0.98]."""
    prev = np.asarray(prev, np.float64)
    H, W = prev.shape
    sigma = noise_sigma(prev, gain, read_noise)
    nxt = prev + rng.normal(0, 1, (H, W)) * sigma
    nxt[:H // 2, :W // 2] = rng.uniform(0.05, 0.95, (H // 2, W // 2))
    nxt[H - H // 2:, W - W // 2:] += 2.4 * sigma[H - H // 2:, W - W // 2:]
    return np.clip(nxt, 0.02, 0.98)


def make_sequence(rng, H, W, n, gain, read_noise):
    """n frames of values in [0, 1] (f64): a noisy smooth scene, then next_frame() of each."""
    frames = [np.clip(noisy(rng, smooth_scene(H, W), gain, read_noise).astype(np.float64), 0.02, 0.98)]
    for _ in range(n - 1):
        frames.append(next_frame(rng, frames[-1], gain, read_noise))
    return frames


def rounding_frame(rng, H, W):
    """(x, h, (gain, read_noise, threshold, max_weight)): a pair whose differences span the whole range and settings whose threshold keeps most weights
    partial, so that y follows every rounding of D, m, qv, k and w (the tap order included)."""
    x = rng.random((H, W)).astype(f32)
    h = (x + rng.uniform(-0.6, 0.6, (H, W))).astype(f32)
    return x, h, (0.01, 0.05, 6.0, 0.75)
