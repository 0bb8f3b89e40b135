"""NumPy restatement of the local tone mapping contract ("Local tone mapping"), shared by the local tone
mapping tests.  It is normative: every f32 operation rounds once (one .astype(float32) each), integers are exact, in the
contract's order.

grids() is the bilateral grid (cnt, sum, Nb, Sb) of one image, gain() the per-pixel gain, local_tonemap() the mapped image.
`mutant` names one deliberate deviation from the contract (MUTANTS); the mutation record and its test use it to show that
the GPU tests' inputs tell each deviation apart.  None is the contract."""
import numpy as np

f32 = np.float32

MUTANTS = ("splat_trunc", "blur_replicate", "lerp_order", "shift_11", "ei_round", "no_clamp", "y0_unclamped")


def _bits(x):
    return np.asarray(x, f32).view(np.int32).astype(np.int64)


class Settings:
    """The settings as the library takes them: mi_isp_local_tonemap holds strength, white, floor and anchor as f32; from
    those values span = li(white), zs = (bins - 1) / span and kq = strength * 4096 are computed in double and rounded
    once."""

    def __init__(self, strength=0.5, white=1.0, floor=2.0 ** -10, anchor=None, cell=32, bins=16, shift=12):
        self.strength = f32(strength)
        self.white = f32(white)
        self.floor = f32(floor)
        self.anchor = self.white if anchor is None else f32(anchor)
        self.cell, self.bins, self.shift = int(cell), int(bins), int(shift)
        self.span = int(self.li(self.white))
        self.zs = f32(float(self.bins - 1) / float(self.span))
        self.kq = f32(float(self.strength) * 4096.0)
        self.la = f32(self.li(self.anchor))

    def li(self, t, clamp=True):
        """2^-11 stops above floor, piecewise linear: the difference of the f32 bit patterns >> 12 (arithmetic)."""
        t = np.asarray(t, f32)
        if clamp:
            t = np.minimum(np.maximum(t, self.floor), self.white)
        return (_bits(t) - _bits(self.floor)) >> self.shift


def as_settings(s, mutant=None):
    """A Settings from a Settings, a dict of its arguments or a LocalTonemap."""
    shift = 11 if mutant == "shift_11" else 12
    if isinstance(s, Settings):
        return Settings(s.strength, s.white, s.floor, s.anchor, s.cell, s.bins, shift)
    if isinstance(s, dict):
        return Settings(**s, shift=shift)
    return Settings(s.strength, s.white, s.floor, s.anchor, s.cell, s.bins, shift)


def log_luma(image, settings, mutant=None):
    """(l, z) of an (H, W, 3) f16 / f32 image: l = li(Y) as int64, z = f32(l) * zs."""
    s = as_settings(settings, mutant)
    v = np.asarray(image).astype(f32)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    Y = (((r + b).astype(f32) * f32(0.25)).astype(f32) + (g * f32(0.5)).astype(f32)).astype(f32)
    l = s.li(Y, clamp=mutant != "no_clamp")
    z = (l.astype(f32) * s.zs).astype(f32)
    return l, z


def grid_shape(H, W, settings):
    s = as_settings(settings)
    return (H + s.cell - 1) // s.cell, (W + s.cell - 1) // s.cell, s.bins


def _blur_axis(a, axis, replicate):
    """The [1 2 1] filter along one axis of an int64 array, zero (or, for the mutant, replicated) outside."""
    a = np.moveaxis(a, axis, 0)
    p = np.concatenate([a[:1] if replicate else np.zeros_like(a[:1]), a,
                        a[-1:] if replicate else np.zeros_like(a[:1])])
    out = p[:-2] + 2 * p[1:-1] + p[2:]
    return np.moveaxis(out, 0, axis)


def grids(image, settings, mutant=None):
    """(cnt, sum, Nb, Sb) of one image, each (GH, GW, bins): the splat counts and sums (uint32) and their blurred f32
    planes."""
    s = as_settings(settings, mutant)
    H, W = image.shape[:2]
    GH, GW, bins = grid_shape(H, W, s)
    l, z = log_luma(image, s, mutant)
    if mutant == "splat_trunc":
        zi = np.minimum(z.astype(np.int64), bins - 1)
    else:
        zi = np.minimum(((z + f32(0.5)).astype(f32)).astype(np.int64), bins - 1)
    if mutant == "no_clamp":                         # (a mutant's bins may leave the grid: keep the scatter in bounds)
        zi = np.clip(zi, 0, bins - 1)
    yy, xx = np.meshgrid(np.arange(H) // s.cell, np.arange(W) // s.cell, indexing="ij")
    flat = ((yy * GW + xx) * bins + zi).reshape(-1)
    cnt = np.bincount(flat, minlength=GH * GW * bins).astype(np.int64)
    sm = np.zeros(GH * GW * bins, np.int64)
    np.add.at(sm, flat, l.reshape(-1))
    cnt, sm = cnt.reshape(GH, GW, bins), sm.reshape(GH, GW, bins)
    bc, bs = cnt, sm
    for axis in range(3):
        bc = _blur_axis(bc, axis, mutant == "blur_replicate")
        bs = _blur_axis(bs, axis, mutant == "blur_replicate")
    return ((cnt & 0xFFFFFFFF).astype(np.uint32), (sm & 0xFFFFFFFF).astype(np.uint32), bc.astype(f32), bs.astype(f32))


def _axis(n, cell, G, mutant=None):
    """(i0, i1, f) of the n pixel centres of an axis with G grid nodes."""
    g = ((np.arange(n).astype(f32) + f32(0.5)).astype(f32) * f32(1.0 / cell)).astype(f32)
    g = np.minimum(np.maximum((g - f32(0.5)).astype(f32), f32(0)), f32(G - 1))
    hi = G - 2 if mutant == "y0_unclamped" else max(G - 2, 0)
    i0 = np.minimum(g.astype(np.int64), hi)
    i1 = np.minimum(i0 + 1, G - 1)
    f = (g - i0.astype(f32)).astype(f32)
    return i0, i1, f


def _lerp(a, b, f):
    return (a + ((b - a).astype(f32) * f).astype(f32)).astype(f32)


def _slice(P, y0, y1, fy, x0, x1, fx, z0, fz, order):
    """The trilinear read of the (GH, GW, bins) f32 plane P for every pixel: lerps along the axes in `order`."""
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    FY = np.broadcast_to(fy[:, None], z0.shape)
    FX = np.broadcast_to(fx[None, :], z0.shape)
    c = {(a, b, d): P[(Y0, Y1)[a], (X0, X1)[b], z0 + d] for a in (0, 1) for b in (0, 1) for d in (0, 1)}
    f = {"y": FY, "x": FX, "z": fz}
    left = ["y", "x", "z"]
    for ax in order:
        k = left.index(ax)
        nxt = {}
        for key in c:
            if key[k] == 0:
                other = key[:k] + (1,) + key[k + 1:]
                nxt[key[:k] + key[k + 1:]] = _lerp(c[key], c[other], f[ax])
        c = nxt
        left.remove(ax)
    return c[()]


def gain(image, settings, mutant=None, planes=None):
    """The (H, W) f32 gain of every pixel; planes: (Nb, Sb) computed before (else from grids())."""
    s = as_settings(settings, mutant)
    H, W = image.shape[:2]
    GH, GW, bins = grid_shape(H, W, s)
    if H * W == 0:
        return np.zeros((H, W), f32)
    Nb, Sb = planes if planes is not None else grids(image, s, mutant)[2:]
    l, z = log_luma(image, s, mutant)
    y0, y1, fy = _axis(H, s.cell, GH, mutant)
    x0, x1, fx = _axis(W, s.cell, GW)
    z0 = np.minimum(z.astype(np.int64), bins - 2)
    if mutant == "no_clamp":
        z0 = np.clip(z0, 0, bins - 2)
    fz = (z - z0.astype(f32)).astype(f32)
    order = "yxz" if mutant == "lerp_order" else "xyz"
    if mutant == "y0_unclamped":                     # (y0 = -1 when GH == 1: a read outside the grid, modelled as NaN)
        Nb, Sb = (np.concatenate([np.full_like(P[:1], np.nan), P]) for P in (Nb, Sb))
        y0, y1 = y0 + 1, y1 + 1
    N = _slice(Nb, y0, y1, fy, x0, x1, fx, z0, fz, order)
    S = _slice(Sb, y0, y1, fy, x0, x1, fx, z0, fz, order)
    with np.errstate(divide="ignore", invalid="ignore"):
        base = np.where(N > 0, (S / N).astype(f32), l.astype(f32))
        e = ((s.la - base).astype(f32) * s.kq).astype(f32)
        if mutant == "ei_round":
            ei = np.rint(e).astype(np.int64)
        else:
            ei = e.astype(np.int64)                  # (truncation toward zero)
    return (np.int64(0x3F800000) + ei).astype(np.int32).view(f32)


def local_tonemap(image, settings, mutant=None):
    """The mapped image, in the image's dtype (f16 or f32)."""
    image = np.asarray(image)
    assert image.ndim == 3 and image.shape[2] == 3 and image.dtype in (np.float16, np.float32)
    if image.size == 0:
        return image.copy()
    g = gain(image, settings, mutant)
    with np.errstate(over="ignore"):
        return (image.astype(f32) * g[..., None]).astype(f32).astype(image.dtype)


# ---- the inputs of the GPU tests (tests/test_gpu_local_tonemap.py), also what the mutation record is measured on ----------
# (H, W, settings): 8 x 8 is one cell (GH = GW = 1); 24 x 40, 66 x 70 and 130 x 66 have partial cells; 72 x 200 takes the
# wide loads (W % 4 == 0) and crosses the 64-pixel region seam of the splat and the tile seam of the apply kernel three
# times along x, 130 rows cross them twice along y; the grids of 130 x 66 and 72 x 200 at cell 8 span several 256-node
# blocks of the blur.  No kernel sweeps its grid, so there is no shape beyond a first sweep; the launches sweep the images
# 32 at a time, which the batch of 33 crosses.
SHAPE_SETTINGS = [
    (8, 8, dict(cell=8, bins=2)),
    (24, 40, dict(cell=16, bins=8)),
    (66, 70, dict(cell=32, bins=16)),
    (130, 66, dict(cell=64, bins=32)),
    (130, 66, dict(cell=8, bins=32, strength=0.3, anchor=0.18)),
    (72, 200, dict(cell=8, bins=16, strength=1.0, floor=2.0 ** -8, white=2.0)),
    (72, 200, dict(cell=32, bins=8, strength=0.05, anchor=0.01)),
    (66, 70, dict(cell=64, bins=2, strength=0.3, anchor=0.18)),
]
CONTENTS = ("wide", "flat", "edge")


def make_image(rng, H, W, content, dtype):
    """A test image.  wide: log-uniform luminances over 14 stops with values below floor, above white, zero and negative;
    flat: one value everywhere (every lane of a wave hits one bin); edge: a 0.01 / 0.8 step with 2 % noise."""
    if content == "flat":
        img = np.full((H, W, 3), 0.05, f32)
    elif content == "edge":
        img = np.where(np.arange(W)[None, :, None] < W // 2, f32(0.01), f32(0.8)) * np.ones((H, 1, 3), f32)
        img = (img * (1 + 0.02 * rng.standard_normal((H, W, 1)))).astype(f32)
    else:
        lum = np.exp2(rng.uniform(-12.0, 1.5, (H, W, 1)))
        img = (lum * rng.uniform(0.5, 1.5, (H, W, 3))).astype(f32)
        kind = rng.random((H, W, 1))
        img = np.where(kind < 0.05, -img, img)                     # negative
        img = np.where((kind >= 0.05) & (kind < 0.08), f32(0), img)
        img = np.where((kind >= 0.08) & (kind < 0.12), f32(1e-6), img)     # below floor
        img = np.where((kind >= 0.12) & (kind < 0.16), img + f32(3.0), img)    # above white
    return img.astype(dtype)


def gpu_test_inputs():
    """[(name, image, settings dict)] of the bit-exact GPU cases, generated the same way every time."""
    out = []
    for i, (H, W, kw) in enumerate(SHAPE_SETTINGS):
        for j, content in enumerate(CONTENTS):
            for dtype in (np.float16, np.float32):
                rng = np.random.default_rng(1000 + 10 * i + j)
                name = f"{H}x{W}-c{kw['cell']}-b{kw['bins']}-{i}-{content}-{np.dtype(dtype).name}"
                out.append((name, make_image(rng, H, W, content, dtype), kw))
    return out
