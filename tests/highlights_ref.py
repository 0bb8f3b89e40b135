"""NumPy f32 restatement of the highlight reconstruction contract ("Highlight reconstruction"), shared by the
highlights tests.  Every intermediate is an np.float32 array and every operation rounds once, in the contract's order.

reconstruct() is y of every raw pixel from the pre-shading, pre-cast values x; route_cfa() the work-dtype CFA the route
hands to the demosaic (before the defect fix-up); make_codes() the test frames: raw codes with clipped blobs over the tile
seams and a corner, isolated clipped pixels of each site and saturated pure colours that must stay as they are."""
import numpy as np

from oracle import isp_oracle as O

f32 = np.float32
COLOURS = O.PIXEL_ORDER                                  # pattern -> the colour (0 R, 1 G, 2 B) of sites 0 .. 3
RB_A = [(-1, 0), (0, -1), (0, 1), (1, 0)]                # the four G neighbours of an R or B site
RB_B = [(-1, -1), (-1, 1), (1, -1), (1, 1)]              # the opposite colour
G_A = [(0, -1), (0, 1)]
G_B = [(-1, 0), (1, 0)]


def site_map(H, W):
    return (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)


def gain_map(wb, pattern, H, W):
    """w[s(q)] of every pixel, (H, W) f32; wb = (w_R, w_G, w_B)."""
    w = np.asarray(wb, f32)
    return w[np.asarray(COLOURS[pattern])][site_map(H, W)]


def green_map(pattern, H, W):
    return np.asarray(COLOURS[pattern])[site_map(H, W)] == 1


def _group_mean(b, kept, offsets):
    """(m, n): the f32 mean of the kept taps' b over `offsets` in order (S starts from the first kept tap), and their count."""
    H, W = b.shape
    bp = np.zeros((H + 2, W + 2), f32)
    kp = np.zeros((H + 2, W + 2), bool)
    bp[1:-1, 1:-1] = b
    kp[1:-1, 1:-1] = kept
    S = np.zeros((H, W), f32)
    n = np.zeros((H, W), np.int32)
    for dr, dc in offsets:
        bq = bp[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]
        kq = kp[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]
        S = np.where(kq, np.where(n > 0, (S + bq).astype(f32), bq), S).astype(f32)
        n = n + kq
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (S / n.astype(f32)).astype(f32)
    return m, n


def reconstruct(x, pattern, wb, mode="rebuild", clip=0.98, excluded=None):
    """y (H, W) f32.  x: (H, W) f32; wb: (w_R, w_G, w_B); excluded: (H, W) bool, the defect map's sites (never a tap; as a
    centre they keep x) or None."""
    x = np.asarray(x)
    assert x.dtype == f32 and x.ndim == 2
    H, W = x.shape
    t = f32(clip)
    w = gain_map(wb, pattern, H, W)
    listed = np.zeros((H, W), bool) if excluded is None else np.asarray(excluded, bool)
    if mode == "clip":
        wmin = np.asarray(wb, f32).min()
        lim = (f32(t * wmin) / w).astype(f32)
        return np.where((x > lim) & ~listed, lim, x).astype(f32)
    assert mode == "rebuild"
    with np.errstate(invalid="ignore", over="ignore"):
        b = (x * w).astype(f32)
        clipped = (x >= t) & ~listed
        kept = ~listed
        green = green_map(pattern, H, W)
        mA_rb, nA_rb = _group_mean(b, kept, RB_A)
        mB_rb, nB_rb = _group_mean(b, kept, RB_B)
        mA_g, nA_g = _group_mean(b, kept, G_A)
        mB_g, nB_g = _group_mean(b, kept, G_B)
        mA, nA = np.where(green, mA_g, mA_rb), np.where(green, nA_g, nA_rb)
        mB, nB = np.where(green, mB_g, mB_rb), np.where(green, nB_g, nB_rb)
        haveA, haveB = nA > 0, nB > 0
        e = np.where(haveA & haveB, np.maximum(mA, mB), np.where(haveA, mA, mB)).astype(f32)
        raise_ = clipped & (haveA | haveB) & (e > b)
        with np.errstate(divide="ignore"):
            cand = np.maximum(x, (e / w).astype(f32))
    return np.where(raise_, cand, x).astype(f32)


def route_cfa(x, pattern, wb, mode, clip, work, gain=None, excluded=None):
    """The route's CFA before the defect fix-up: cast_work(y * g), or cast_work(y) without a grid."""
    y = reconstruct(x, pattern, wb, mode, clip, excluded)
    return O.cast_out(y if gain is None else (y * np.asarray(gain, f32)).astype(f32), work)


# ---- the test frames ---------------------------------------------------------------------------------------------------
def make_codes(rng, H, W, top, lo, pattern=O.RGGB, clipped=True):
    """(H, W) u16 raw codes in 0 .. top of a smooth-plus-noise scene below the clip level.  clipped: codes in lo .. top
    (lo: the smallest code the caller's clip level calls clipped) in blobs straddling rows and columns 63/64 (where the
    frame has them) and the frame's corners, in a band of rows, in a ragged field of isolated pixels of every site, and as
    saturated pure colours (one colour at `top` among dark neighbours), which the operator leaves alone."""
    r = np.arange(H)[:, None] / max(H, 1)
    c = np.arange(W)[None, :] / max(W, 1)
    base = 0.15 + 0.5 * (0.5 + 0.5 * np.sin(5.0 * r + 1.0)) * (0.5 + 0.5 * np.cos(7.0 * c))
    v = np.clip(base + rng.normal(0, 0.02, (H, W)), 0.02, 0.8)
    codes = np.rint(v * lo).astype(np.uint16)
    if not clipped:
        return codes
    sat = np.zeros((H, W), bool)
    sat[:min(H, 5), :min(W, 7)] = True                   # the top-left corner
    if H > 8 and W > 8:
        sat[H - 3:, W - 4:] = True                       # the bottom-right corner
    for (r0, r1, c0, c1) in [(58, 70, 10, 22), (20, 30, 59, 69), (60, 68, 60, 68), (124, 134, 30, 40)]:
        sat[r0:min(r1, H), c0:min(c1, W)] = True         # the tile seams
    if H >= 32:
        sat[H // 2:H // 2 + H // 8] = True               # a band of rows
    if H * W >= 64:
        sat |= rng.random((H, W)) < 0.04                 # isolated pixels of every site, pairs, small clusters
    codes[sat] = rng.integers(lo, top + 1, int(sat.sum()))
    cols = np.asarray(COLOURS[pattern])[site_map(H, W)]
    if H >= 16 and W >= 16:
        for s in range(4):                               # one isolated clipped pixel per site among bright neighbours
            rr, cc = 8 + (s >> 1), 12 + 6 * s + (s & 1)
            if cc + 2 < W:
                codes[rr - 1:rr + 2, cc - 1:cc + 2] = int(0.9 * lo)
                codes[rr, cc] = top
        for k, colour in enumerate((0, 1, 2)):           # saturated pure colours
            r0, c0 = min(36, H - 8), 4 + 10 * k
            if c0 + 8 <= W:
                patch = codes[r0:r0 + 8, c0:c0 + 8]
                patch[...] = int(0.05 * lo)
                patch[cols[r0:r0 + 8, c0:c0 + 8] == colour] = top
    return codes


def coverage(x, y, clip, H, W):
    """(fraction of pixels raised, per site: clipped pixels left unchanged) - what a frame of H * W >= 4096 must show."""
    raised = y > x
    kept = (x >= f32(clip)) & (y == x)
    s = site_map(H, W)
    return raised.mean(), [int((kept & (s == k)).sum()) for k in range(4)]
