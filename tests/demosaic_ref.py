"""The direction-adaptive demosaic's contract ("Directional demosaic"), restated in NumPy f32.

Written for clarity, not speed: every quantity is an array over the CFA extended by PAD pixels on every side, A(r + dr,
c + dc) is `at(A, dr, dc)`, and every line is one f32 operation per element in the order the contract gives.  The
extension is the mirror that does not repeat the edge sample (index i folds with period 2 (n - 1)), which keeps the Bayer
phase, so nothing below has a border case.

`mutant=` builds a deliberately wrong operator (MUTANTS); tests/test_demosaic_cpu.py shows that each one fails a vector.
"""
import numpy as np

from oracle import isp_oracle as O

f32 = np.float32
PAD = 16                                    # >= the stencil's reach (4 before, 8 after) plus what the rolls wrap around
MUTANTS = ("hv_swap", "tie_flip", "window_mirror", "clamp_edge", "step5_across")
HALF, QUARTER, THREE = f32(0.5), f32(0.25), f32(3.0)


def fold(i, n):
    """Index i of the mirror extension of n >= 2 samples: -1 -> 1, n -> n - 2, repeatedly."""
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def extend(cfa, mutant=None):
    """X over [-PAD, H + PAD) x [-PAD, W + PAD), f32."""
    H, W = cfa.shape
    r, c = np.arange(-PAD, H + PAD), np.arange(-PAD, W + PAD)
    if mutant == "clamp_edge":
        rr, cc = np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)
    else:
        rr, cc = fold(r, H), fold(c, W)
    return cfa.astype(f32)[np.ix_(rr, cc)]


def at(A, dr, dc):
    """A(r + dr, c + dc) at every (r, c) (what wraps around stays inside the padding)."""
    return np.roll(A, (-dr, -dc), axis=(0, 1))


def site_masks(shape, pattern):
    """(green, red, blue) boolean masks of the extended plane."""
    Hp, Wp = shape
    r, c = np.meshgrid(np.arange(-PAD, Hp - PAD), np.arange(-PAD, Wp - PAD), indexing="ij")
    colour = np.asarray(O.PIXEL_ORDER[pattern])[(r & 1) * 2 + (c & 1)]
    return colour == 1, colour == 0, colour == 2


def steps123(cfa, pattern, mutant=None):
    """(X, G at every site (X itself at green sites), horizontal, GH, GV, green, red, blue) on the extended plane."""
    X = extend(cfa, mutant)
    green, red, blue = site_masks(X.shape, pattern)
    # step 1: the directional estimates
    eh = (at(X, 0, -1) + at(X, 0, 1)) * HALF + ((X + X) - (at(X, 0, -2) + at(X, 0, 2))) * QUARTER
    ev = (at(X, -1, 0) + at(X, 1, 0)) * HALF + ((X + X) - (at(X, -2, 0) + at(X, 2, 0))) * QUARTER
    if mutant == "hv_swap":
        eh, ev = ev, eh
    CH = np.where(green, eh - X, X - eh)    # chroma minus green
    CV = np.where(green, ev - X, X - ev)
    # step 2: the classifier
    DH = np.abs(CH - at(CH, 0, 2))
    DV = np.abs(CV - at(CV, 2, 0))
    k = -1 if mutant == "window_mirror" else 1
    dH = at(DH, -2, 0)                                          # row r - 2
    dH = dH + at(DH, -2, 2 * k)
    dH = dH + at(DH, -1, 1 * k)                                 # row r - 1
    dH = dH + THREE * DH                                        # row r
    dH = dH + THREE * at(DH, 0, 2 * k)
    dH = dH + at(DH, 1, 1 * k)                                  # row r + 1
    dH = dH + at(DH, 2, 0)                                      # row r + 2
    dH = dH + at(DH, 2, 2 * k)
    dV = at(DV, 0, -2)                                          # the transpose: column c - 2
    dV = dV + at(DV, 2 * k, -2)
    dV = dV + at(DV, 1 * k, -1)
    dV = dV + THREE * DV
    dV = dV + THREE * at(DV, 2 * k, 0)
    dV = dV + at(DV, 1 * k, 1)
    dV = dV + at(DV, 0, 2)
    dV = dV + at(DV, 2 * k, 2)
    horizontal = dV > dH if mutant == "tie_flip" else dV >= dH
    # step 3: green at the red and blue sites
    G = np.where(green, X, np.where(horizontal, eh, ev))
    return X, G, horizontal, eh, ev, green, red, blue


def planes(cfa, pattern=O.RGGB, mutant=None):
    """The (H, W, 3) f32 image of steps 1 - 5, before the epilogue."""
    H, W = cfa.shape
    assert H >= 2 and W >= 2 and H % 2 == 0 and W % 2 == 0
    X, G, horizontal, _, _, green, red, blue = steps123(cfa, pattern, mutant)
    # step 4: red and blue at the green sites, from the chroma K - G of the two neighbours that hold K
    D = X - G                                                   # K(q) - G(q) at a red or blue site q
    Krow = X + (at(D, 0, -1) + at(D, 0, 1)) * HALF
    Kcol = X + (at(D, -1, 0) + at(D, 1, 0)) * HALF
    red_row = at(red, 0, 1)                                     # at a green site: its row neighbours are red
    Rg = np.where(red_row, Krow, Kcol)
    Bg = np.where(red_row, Kcol, Krow)
    # step 5: red at the blue sites, blue at the red sites, from R - B of the green neighbours along the decision
    RB = Rg - Bg
    dh = (at(RB, 0, -1) + at(RB, 0, 1)) * HALF
    dv = (at(RB, -1, 0) + at(RB, 1, 0)) * HALF
    along = ~horizontal if mutant == "step5_across" else horizontal
    d = np.where(along, dh, dv)
    R = np.where(green, Rg, np.where(red, X, X + d))
    B = np.where(green, Bg, np.where(blue, X, X - d))
    return np.stack([R, G, B], axis=-1)[PAD:PAD + H, PAD:PAD + W]


def finish(rgb, correct_colors=None, dtype="f32"):
    """Step 6, mi_isp_demosaic's epilogue: the sequential f32 dot, clamp01, * scale(dtype), the cast."""
    out = rgb.astype(f32)
    if correct_colors is not None:
        M = np.asarray(correct_colors, dtype=np.float64).reshape(3, 3).astype(f32)
        out = np.stack([(M[k, 0] * out[..., 0] + M[k, 1] * out[..., 1]) + M[k, 2] * out[..., 2] for k in range(3)], axis=-1)
    out = np.minimum(np.maximum(out, f32(0)), f32(1))
    return O.cast_out(out * f32(O.SCALE[dtype]), dtype)


def directional(cfa, pattern=O.RGGB, correct_colors=None, dtype=None, mutant=None):
    """The operator on an f16 or f32 CFA; dtype: the output's ("u8", "u16", "f16", "f32"; None: the CFA's)."""
    assert cfa.dtype in (np.float16, np.float32)
    return finish(planes(cfa, pattern, mutant), correct_colors, O.dtype_name(cfa) if dtype is None else dtype)


def stripes_codes(shape, seed=0):
    """The GPU tests' frames as 12-bit codes: the left half vertical stripes, the right half horizontal stripes, both of
    ~3 px period and +-0.3 around 0.5, plus sigma = 0.05 noise: both decisions and both estimates are busy."""
    H, W = shape
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    wave = np.where(c < W // 2, np.sin(2 * np.pi * c / 3.0), np.sin(2 * np.pi * r / 3.0))
    x = 0.5 + 0.3 * wave + rng.normal(0.0, 0.05, size=(H, W))
    return np.clip(np.round(x * 4095.0), 0, 4095).astype(np.uint16)


def stripes_cfa(shape, seed=0, dtype=np.float32):
    """The same frame as a normalised CFA of `dtype`."""
    return (stripes_codes(shape, seed).astype(f32) * f32(1.0 / 4095.0)).astype(dtype)


# the tile of the kernel (csrc/isp_demosaic_dir.h) and the shapes the GPU tests use: the degenerate ones, one tile, one tile
# + 2 and two tiles + 2 each way (every seam and a ragged last tile); BIG are those of 4096 pixels or more, whose generated
# frames must meet the coverage condition (tests/test_demosaic_cpu.py)
TILE_H, TILE_W = 32, 64
SHAPES = [(2, 2), (2, 6), (4, 2), (6, 4), (TILE_H, TILE_W), (TILE_H + 2, TILE_W + 2), (2 * TILE_H + 2, 2 * TILE_W + 2)]
BIG = [s for s in SHAPES if s[0] * s[1] >= 4096]
SEEDS = range(4)                            # the seeds the GPU tests draw their frames with


def assert_covered(cfa, pattern=O.RGGB, what=""):
    """The coverage condition, on the reference alone: a frame of 4096 pixels or more decides each way at >= 25 % of its
    red / blue sites and has GH != GV in f16 at >= 50 % of them."""
    if cfa.size >= 4096:
        h, v, differ = coverage(cfa, pattern)
        assert h >= 0.25 and v >= 0.25 and differ >= 0.5, f"{what}: the frame does not exercise the operator ({h}, {v}, {differ})"


def coverage(cfa, pattern=O.RGGB):
    """(the share of the red / blue sites decided horizontal, the share decided vertical, the share where GH and GV differ
    after rounding to f16)."""
    H, W = cfa.shape
    _, _, horizontal, eh, ev, green, _, _ = steps123(cfa, pattern)
    crop = (slice(PAD, PAD + H), slice(PAD, PAD + W))
    rb = ~green[crop]
    hz = horizontal[crop][rb]
    with np.errstate(over="ignore"):
        differ = eh[crop][rb].astype(np.float16) != ev[crop][rb].astype(np.float16)
    return float(hz.mean()), float(1.0 - hz.mean()), float(differ.mean())
