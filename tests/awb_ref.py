"""NumPy restatement of the auto white balance contract ("Auto white balance"), shared by the AWB tests.

stats() is the statistics of one frame from its pre-cast values x (and the user's per-pixel gains), update() one update
of the gray-world loop, effective() the grid E the loaders apply.  Every f32 operation is rounded as the contract says;
the update runs in Python floats (f64, never fused)."""
import numpy as np

f32 = np.float32
# colour (0 R, 1 G, 2 B) of CFA site s = (row & 1) * 2 + (col & 1) under each demosaic pattern (RGGB, GRBG, GBRG, BGGR)
SITE_COLOUR = {0: (0, 1, 1, 2), 1: (1, 0, 2, 1), 2: (1, 2, 0, 1), 3: (2, 1, 1, 0)}


def stats(x, g=None, clip=0.95, floor=0.02, stride=4):
    """(P0, P1, P2, P3, n) as Python ints for one frame: x and g (H, W) f32 (g None: no user grid)."""
    x = np.asarray(x, f32)
    H, W = x.shape
    xs = x if g is None else (x * np.asarray(g, f32)).astype(f32)

    def quads(a):
        return a[:H // 2 * 2, :W // 2 * 2].reshape(H // 2, 2, W // 2, 2).transpose(0, 2, 1, 3)[::stride, ::stride]

    xq, sq = quads(x), quads(xs)
    with np.errstate(invalid="ignore"):
        keep = (xq < f32(clip)).all(axis=(2, 3)) & (xq.max(axis=(2, 3)) >= f32(floor))
        q = np.rint(np.minimum(np.maximum(sq, f32(0)), f32(2.0 ** 15)) * f32(2.0 ** 24)).astype(f32)
    kept = q[keep]                                           # (k, 2, 2)
    P = [int(kept[:, s >> 1, s & 1].astype(np.uint64).sum(dtype=np.uint64)) for s in range(4)]
    return P + [int(keep.sum())]


def add(*rows):
    return [sum(int(r[k]) for r in rows) for k in range(5)]


class State:
    """The loop's device state: S (3 f64), valid, gains (3 f32)."""

    def __init__(self, white_balance):
        self.S = [0.0, 0.0, 0.0]
        self.valid = False
        self.gains = np.asarray(white_balance, np.float64).astype(f32)

    def update(self, P, pattern, moving_alpha):
        """One update from the summed pending row P (5 ints); t = 1 - moving_alpha, 0 for the first update."""
        n = int(P[4])
        if n == 0:
            return self
        m = [(float(int(P[s])) * 2.0 ** -24) / float(n) for s in range(4)]
        col = SITE_COLOUR[int(pattern)]
        greens = [m[s] for s in range(4) if col[s] == 1]
        c = [m[col.index(0)], (greens[0] + greens[1]) * 0.5, m[col.index(2)]]
        t = (1.0 - moving_alpha) if self.valid else 0.0
        self.S = [c[k] + t * (self.S[k] - c[k]) for k in range(3)]
        self.valid = True
        g = self.gains.copy()
        SR, SG, SB = self.S
        if SG > 0 and SR > 0:
            g[0] = f32(min(max(SG / SR, 0.125), 8.0))
        if SG > 0 and SB > 0:
            g[2] = f32(min(max(SG / SB, 0.125), 8.0))
        g[1] = f32(1.0)
        self.gains = g
        return self


def effective(gains, pattern, user=None):
    """E (4, Gh, Gw) f32: the user's grid (sites 1 or 4; None: 2 x 2 ones) times each site's colour gain."""
    if user is None:
        U = np.ones((1, 2, 2), f32)
    else:
        U = np.asarray(user, f32)
        U = U[None] if U.ndim == 2 else U
    col = SITE_COLOUR[int(pattern)]
    return np.stack([(U[s if U.shape[0] == 4 else 0] * f32(gains[col[s]])).astype(f32) for s in range(4)])
