"""The directional demosaic without a GPU: the restatement (tests/demosaic_ref.py) against vectors worked out by hand,
its tie rule and pattern symmetry, the coverage condition of the frames the GPU tests use, its quality against the 13-tap
filter, the C entry points' host-side refusals, the Python settings - and that each mutant of the restatement (R.MUTANTS;
the record is profiles/demosaic_dir_mutations.txt) fails one of the vectors."""
import ctypes

import numpy as np
import pytest

from oracle import isp_oracle as O
from tests import demosaic_ref as R
from tests.util import assert_exact

f32 = np.float32
HALF = f32(0.5)


def nyquist(shape, vertical, a=0.25, b=0.75, growth=0.0):
    """A grey scene of one-pixel-wide stripes (the values alternate between a and b, the swing grows by `growth` per
    stripe), vertical or horizontal; grey: the CFA holds the scene itself."""
    H, W = shape
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    k = c if vertical else r
    mid, swing = (a + b) / 2, (b - a) / 2
    return (mid + np.where(k % 2 == 0, -1.0, 1.0) * (swing + growth * k)).astype(f32)


# ---- the vectors, one function per mutant-catching property -------------------------------------------------------------
def vector_flat(mutant=None):
    for pattern in range(4):
        out = R.planes(np.full((6, 8), 0.25, f32), pattern, mutant)
        assert_exact(out, np.full((6, 8, 3), 0.25, f32), f"flat, pattern {pattern}")


def vector_horizontal_stripes(mutant=None):
    """Rows of a grey scene: eh = X exactly, so CH = 0, dH = 0 <= dV: every site is horizontal and the scene comes back
    exactly, border included (the mirror of a row-only scene is row-only)."""
    for pattern in range(4):
        s = nyquist((12, 16), vertical=False)
        assert_exact(R.planes(s, pattern, mutant), np.repeat(s[..., None], 3, axis=2), f"horizontal stripes, pattern {pattern}")


def vector_vertical_stripes(mutant=None):
    """Columns of a grey scene whose swing grows: ev = X exactly, so CV = 0 and dV = 0 < dH: every site is vertical and the
    scene comes back exactly."""
    for pattern in range(4):
        s = nyquist((12, 16), vertical=True, growth=0.01)
        assert_exact(R.planes(s, pattern, mutant), np.repeat(s[..., None], 3, axis=2), f"vertical stripes, pattern {pattern}")


def vector_tie(mutant=None):
    """Vertical stripes of a CONSTANT swing alias perfectly: CH is the same at every site and CV is 0, so dH = dV = 0 at
    every site.  The tie goes to horizontal: green at a red / blue site is eh, the neighbour stripes' value."""
    s = nyquist((12, 16), vertical=True)
    _, G, horizontal, eh, ev, green, _, _ = R.steps123(s, O.RGGB, mutant)
    assert horizontal.all(), "a tie goes to horizontal"
    crop = (slice(R.PAD, R.PAD + 12), slice(R.PAD, R.PAD + 16))
    other = nyquist((12, 16), vertical=True, a=0.75, b=0.25)                    # (the neighbour stripes' value)
    want = np.where(green[crop], s, other)
    assert_exact(R.planes(s, O.RGGB, mutant)[..., 1], want, "green under the tie rule")


def vector_2x2(mutant=None):
    """RGGB [[.1 .2] [.3 .4]]: the extended plane has period 2 both ways, every DH and DV is 0, every site is horizontal."""
    a, b, c, d = f32(0.1), f32(0.2), f32(0.3), f32(0.4)
    g00 = (b + b) * HALF + ((a + a) - (a + a)) * f32(0.25)                      # eh at the red site: its row neighbours
    g11 = (c + c) * HALF + ((d + d) - (d + d)) * f32(0.25)                      # eh at the blue site
    r01 = b + ((a - g00) + (a - g00)) * HALF                                    # green (0, 1): red from its row ...
    b01 = b + ((d - g11) + (d - g11)) * HALF                                    # ... blue from its column
    b10 = c + ((d - g11) + (d - g11)) * HALF                                    # green (1, 0): blue from its row ...
    r10 = c + ((a - g00) + (a - g00)) * HALF                                    # ... red from its column
    d00 = ((r01 - b01) + (r01 - b01)) * HALF                                    # red site, horizontal: both neighbours are (0, 1)
    d11 = ((r10 - b10) + (r10 - b10)) * HALF
    want = np.array([[[a, g00, a - d00], [r01, b, b01]], [[r10, c, b10], [d + d11, g11, d]]], f32)
    assert_exact(R.planes(np.array([[a, b], [c, d]], f32), O.RGGB, mutant), want, "2 x 2")


ROW0 = [f32(v) for v in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)]
ROW1 = ROW0[::-1]


def vector_2x6(mutant=None):
    """RGGB rows [.1 .. .6] and [.6 .. .1]: columns -4 .. 9 fold to 4 3 2 1 | 0 .. 5 | 4 3 2 1, rows have period 2, so every
    DV is 0 and every site with dH > 0 is vertical.  Pixel (0, 0) by hand."""
    cfa = np.array([ROW0, ROW1], f32)
    X = R.extend(cfa, mutant)
    cols = [4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 4, 3, 2, 1]
    assert_exact(X[R.PAD, R.PAD - 4:R.PAD + 10], cfa[0, cols], "the mirror of row 0")
    assert_exact(X[R.PAD - 1, R.PAD - 4:R.PAD + 10], cfa[1, cols], "row -1 is row 1")
    x00, x10, x01, x11 = ROW0[0], ROW1[0], ROW0[1], ROW1[1]
    g00 = (x10 + x10) * HALF + ((x00 + x00) - (x00 + x00)) * f32(0.25)          # ev at the red site (0, 0)
    g11 = (x01 + x01) * HALF + ((x11 + x11) - (x11 + x11)) * f32(0.25)          # ev at the blue site (1, 1) = (1, -1)
    b10 = x10 + ((x11 - g11) + (x11 - g11)) * HALF                              # green (1, 0): blue from (1, -1) and (1, 1)
    r10 = x10 + ((x00 - g00) + (x00 - g00)) * HALF                              # ... red from (0, 0) and (2, 0)
    d = ((r10 - b10) + (r10 - b10)) * HALF                                      # (0, 0) is vertical: (-1, 0) and (1, 0)
    out = R.planes(cfa, O.RGGB, mutant)
    assert_exact(out[0, 0], np.array([x00, g00, x00 - d], f32), "2 x 6, pixel (0, 0)")
    assert float(g00) == float(x10) and abs(float(out[0, 0, 2]) - 0.9) < 1e-6


def vector_window(mutant=None):
    """A step that only the classifier's look-ahead sees: flat but for columns >= c + 3 of one row pair, the site at
    column c decides vertical because its window reaches to c + 4, and would tie (horizontal) with the window mirrored."""
    cfa = np.full((16, 24), 0.5, f32)
    cfa[:, 11:] = 0.9                                                           # a vertical edge between columns 10 and 11
    _, _, horizontal, _, _, green, _, _ = R.steps123(cfa, O.RGGB, mutant)
    hz = horizontal[R.PAD:R.PAD + 16, R.PAD:R.PAD + 24]
    # the red site (8, 8): DH(r, 8) compares columns 8 and 10 (equal), DH(r, 10) columns 10 and 12 (the edge): dH > 0 = dV
    assert not hz[8, 8], "the window reaches two columns ahead"
    # the red site (8, 14): its window covers columns 14 .. 18, all past the edge: a tie
    assert hz[8, 14]


def vector_step5(mutant=None):
    """A scene of vertical colour stripes (R - B alternates along the row): every site is vertical, so step 5 must take
    R - B from the column neighbours; across the decision it would mix the stripes' colours."""
    H, W = 12, 16
    c = np.arange(W)[None, :].repeat(H, 0)
    img = np.stack([0.5 + 0.2 * np.sin(c * 0.9), np.full((H, W), 0.5), 0.5 + 0.2 * np.cos(c * 1.3)], -1).astype(f32)
    cfa = O.rgb_to_bayer(img, O.RGGB)
    _, _, horizontal, _, _, green, _, _ = R.steps123(cfa, O.RGGB)
    assert not horizontal[R.PAD:R.PAD + H, R.PAD:R.PAD + W][~green[R.PAD:R.PAD + H, R.PAD:R.PAD + W]].any()
    out = R.planes(cfa, O.RGGB, mutant)
    # every column of the image is constant (the scene and its mirror are column-only; vertical interpolation keeps that)
    assert_exact(out, np.repeat(out[:1], H, axis=0), "vertical decisions keep a column-only scene column-only")


VECTORS = [vector_flat, vector_horizontal_stripes, vector_vertical_stripes, vector_tie, vector_2x2, vector_2x6, vector_window,
           vector_step5]


@pytest.mark.parametrize("vector", VECTORS, ids=lambda f: f.__name__)
def test_hand_derived_vectors(vector):
    vector()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_a_vector(mutant):
    """H/V swapped, the tie flipped, the classifier window mirrored, clamp-to-edge for the mirror, step 5 across the
    decision: each is caught by at least one vector."""
    caught = []
    for vector in VECTORS:
        try:
            vector(mutant)
        except AssertionError:
            caught.append(vector.__name__)
    assert caught, f"no vector notices the mutant {mutant}"


# ---- symmetry, coverage, quality ---------------------------------------------------------------------------------------
def test_the_four_patterns_agree_under_shifts(rng):
    """A window of an RGGB frame that starts at (dr, dc) is a frame of the pattern with that phase: away from the borders
    (8 pixels: the stencil's reach) the two demosaics are the same numbers."""
    H, W = 40, 48
    big = (0.1 + 0.8 * rng.random((H + 2, W + 2))).astype(f32)
    full = R.planes(big, O.RGGB)
    for pattern, (dr, dc) in {O.RGGB: (0, 0), O.GRBG: (0, 1), O.GBRG: (1, 0), O.BGGR: (1, 1)}.items():
        part = R.planes(big[dr:dr + H, dc:dc + W], pattern)
        assert_exact(part[8:-8, 8:-8], full[dr + 8:dr + H - 8, dc + 8:dc + W - 8], f"pattern {pattern}")


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", R.BIG)
def test_the_generated_frames_meet_the_coverage_condition(shape, dtype):
    """A condition on the GPU tests' inputs, on the reference alone: each direction at >= 25 % of the red / blue sites,
    GH != GV in f16 at >= 50 % of them."""
    for seed in R.SEEDS:
        for pattern in range(4):
            R.assert_covered(R.stripes_cfa(shape, seed, dtype), pattern, f"{shape} seed {seed} pattern {pattern}")
    for shape_ in [(64, 64), (66, 70), (130, 66)]:
        h, v, differ = R.coverage(R.stripes_cfa(shape_))
        assert h >= 0.25 and v >= 0.25 and differ >= 0.5


def psnr(a, b, border=8):
    d = a[border:-border, border:-border].astype(np.float64) - b[border:-border, border:-border].astype(np.float64)
    return 10.0 * np.log10(1.0 / np.mean(d * d))


def scenes():
    H, W = 96, 128
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    zone = 0.5 + 0.5 * np.cos(np.pi * ((r - H / 2) ** 2 + (c - W / 2) ** 2) / (2 * W))
    bars = 0.5 + 0.4 * np.sign(np.sin(2 * np.pi * (c + 0.15 * r) / 7.0))
    return {name: np.stack([g, 0.8 * g + 0.1, 0.6 * g + 0.2], -1).astype(f32) for name, g in (("zone plate", zone), ("bars", bars))}


@pytest.mark.parametrize("name", ["zone plate", "bars"])
def test_quality_is_above_the_13_tap_filter(name):
    """Mosaicked through the oracle and scored against the source, 8-pixel border excluded: strictly above the 13-tap
    filter's PSNR on the same CFA (measured: zone plate 27.48 -> 28.33 dB, bars 19.59 -> 24.09 dB)."""
    img = scenes()[name]
    cfa = O.rgb_to_bayer(img, O.RGGB)
    linear, directional = psnr(O.bayer_to_rgb(cfa, O.RGGB), img), psnr(R.directional(cfa, O.RGGB), img)
    print(f"{name}: 13-tap {linear:.2f} dB, directional {directional:.2f} dB")
    assert directional > linear


def test_the_epilogue_is_the_13_tap_filters(rng):
    """Step 6 on its own: the matrix, the clamp, the scale and the cast of O.bayer_to_rgb."""
    rgb = (rng.random((4, 6, 3)) * 1.4 - 0.2).astype(f32)
    M = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
    m = M.astype(f32)
    for dtype in ("u8", "u16", "f16", "f32"):
        dot = np.stack([(m[k, 0] * rgb[..., 0] + m[k, 1] * rgb[..., 1]) + m[k, 2] * rgb[..., 2] for k in range(3)], -1)
        want = O.cast_out(np.clip(dot, 0, 1) * f32(O.SCALE[dtype]), dtype)
        assert_exact(R.finish(rgb, M, dtype), want, dtype)
        assert_exact(R.finish(rgb, None, dtype), O.cast_out(np.clip(rgb, 0, 1) * f32(O.SCALE[dtype]), dtype), dtype)


# ---- the C entry points' host-side checks --------------------------------------------------------------------------------
def test_c_entry_points_reject_bad_arguments_before_any_launch():
    from taichi_image_amd import _native
    L = _native.lib()
    a, b = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    pa, pb = ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p)
    F16, F32, U8 = _native.MI_F16, _native.MI_F32, _native.MI_U8

    def rejected(rc, text):
        err = L.mi_isp_last_error()
        assert rc != 0 and b"demosaic_directional" in err and text.encode() in err, err

    cfa = lambda **kw: L.mi_isp_demosaic_directional_cfa(  # noqa: E731
        kw.get("src", pa), kw.get("dst", pb), kw.get("H", 4), kw.get("W", 4), kw.get("i", F32), kw.get("o", F32),
        kw.get("pattern", 0), None, None)
    rejected(cfa(src=None), "null pointer")
    rejected(cfa(dst=None), "null pointer")
    for H, W in ((3, 4), (4, 5), (0, 4), (4, 0), (-2, 4)):
        rejected(cfa(H=H, W=W), f"even size >= 2, got {H}x{W}")
    rejected(cfa(i=U8), "must be f16 or f32")
    rejected(cfa(i=_native.MI_U16), "must be f16 or f32")
    rejected(cfa(o=4), "bad output dtype 4")
    rejected(cfa(pattern=4), "bad pattern 4")
    rejected(cfa(pattern=-1), "bad pattern -1")

    one, out = (ctypes.c_void_p * 1)(pa), (ctypes.c_void_p * 1)(pb)
    none = (ctypes.c_void_p * 1)(None)
    same = (ctypes.c_void_p * 1)(pa)

    def args(kw, rgb):
        head = (kw.get("srcs", one), kw.get("dsts", out), kw.get("n", 1), kw.get("H", 4), kw.get("W", 4),
                kw.get("kind", _native.MI_RAW_32F), kw.get("ids", 0), kw.get("work", F32))
        tail = (kw.get("levels"), kw.get("shading"))
        return head + ((kw.get("pattern", 0),) if rgb else ()) + tail + ((None,) if rgb else ()) + (None,)

    raw = lambda **kw: L.mi_isp_demosaic_directional_raw_batch(*args(kw, True))  # noqa: E731
    dec = lambda **kw: L.mi_isp_raw_cfa_batch(*args(kw, False))                  # noqa: E731
    for fn in (raw, dec):
        rejected(fn(n=-1), "with -1 frames")
        rejected(fn(srcs=None), "null frame list")
        rejected(fn(dsts=None), "null frame list")
        rejected(fn(srcs=none), "frame 0 has a null pointer")
        rejected(fn(dsts=same), "must not overwrite its source")
        rejected(fn(H=3), "even size >= 2, got 3x4")
        rejected(fn(W=0), "even size >= 2, got 4x0")
        rejected(fn(work=U8), "work dtype must be f16 or f32")
        rejected(fn(kind=5), "source kind 5")
        rejected(fn(kind=-1), "source kind -1")
        rejected(fn(ids=1), "IDS layout")
        rejected(fn(levels=_native.levels_arg([0, 0, 0, 0], 4095)), "levels apply to u16 codes only")
        assert fn(kind=_native.MI_RAW_16U, levels=_native.levels_arg([0, 0, 0, 0], 0)) != 0
        assert b"white level" in L.mi_isp_last_error()                           # (the existing checker's text)
        assert fn(shading=_native.Shading(pa, 3, 2, 2)) != 0
        assert b"shading grid" in L.mi_isp_last_error()
        # n == 0 is a successful no-op, whatever the lists
        assert fn(n=0) == 0 and fn(n=0, srcs=None, dsts=None) == 0
    rejected(raw(pattern=7), "bad pattern 7")
    # a pointer that is not aligned to its element (made-up addresses inside a and b: nothing is launched)
    off = lambda p, n: ctypes.c_void_p(p.value + n)  # noqa: E731
    U16 = _native.MI_U16
    for o, n in ((F32, 1), (F32, 2), (F16, 1), (U16, 1), (F16, 3)):
        rejected(cfa(dst=off(pb, n), o=o), "the CFA or the image not aligned to its element")
    for i, n in ((F32, 2), (F16, 1)):
        rejected(cfa(src=off(pa, n), i=i), "the CFA or the image not aligned to its element")
    for fn in (raw, dec):
        for work, n in ((F32, 2), (F32, 1), (F16, 1)):
            rejected(fn(dsts=(ctypes.c_void_p * 1)(off(pb, n)), work=work), "frame 0 not aligned to its element")
        for kind, n in ((_native.MI_RAW_32F, 2), (_native.MI_RAW_16U, 1), (_native.MI_RAW_16F, 1)):
            rejected(fn(srcs=(ctypes.c_void_p * 1)(off(pa, n)), kind=kind), "frame 0 not aligned to its element")
        two = (ctypes.c_void_p * 2)(pa, off(pa, 34))
        rejected(fn(srcs=two, dsts=(ctypes.c_void_p * 2)(pb, off(pb, 32)), n=2), "frame 1 not aligned to its element")
    assert L.mi_isp_version() == 1900


# ---- Python --------------------------------------------------------------------------------------------------------------
def test_demosaic_settings_and_set():
    import taichi_image_amd as ti
    from taichi_image_amd import demosaic
    assert ti.Demosaic is demosaic.Demosaic and ti.demosaic is demosaic
    assert ti.Demosaic().method == "directional" and ti.Demosaic().is_directional
    assert not ti.Demosaic("malvar").is_directional
    assert ti.Demosaic("directional") == ti.Demosaic() and hash(ti.Demosaic()) == hash(ti.Demosaic("directional"))
    for bad in ("menon", "", None, 1):
        with pytest.raises(ValueError, match="method"):
            ti.Demosaic(bad)
    with pytest.raises(Exception):
        ti.Demosaic().method = "malvar"                                          # frozen
    assert demosaic.check_demosaic(None) is None and demosaic.check_demosaic(ti.Demosaic()) == ti.Demosaic()
    for bad in ("directional", True, 1):
        with pytest.raises(ValueError, match="demosaic"):
            demosaic.check_demosaic(bad)
        with pytest.raises(ValueError, match="demosaic"):
            ti.Camera16(ti.BayerPattern.RGGB, demosaic=bad)
    isp = ti.Camera32(ti.BayerPattern.GRBG)
    assert isp.demosaic is None and not isp._directional()
    isp.set(demosaic=ti.Demosaic())
    assert isp.demosaic == ti.Demosaic() and isp._directional()
    isp.set(moving_alpha=0.3)                                                    # (None leaves it)
    assert isp.demosaic == ti.Demosaic()
    isp.set(demosaic=ti.Demosaic("malvar"))
    assert isp.demosaic.method == "malvar" and not isp._directional()
    with pytest.raises(ValueError, match="demosaic"):
        isp.set(demosaic="directional")
    assert isp.demosaic.method == "malvar"
    isp.set(demosaic=False)
    assert isp.demosaic is None
    # directional() checks its arguments before it asks for a device
    with pytest.raises(ValueError, match="f16 or f32"):
        demosaic.directional(np.zeros((4, 4), np.uint16))
    with pytest.raises(ValueError, match="f16 or f32"):
        demosaic.directional(np.zeros((4, 4), np.float64))
    with pytest.raises(ValueError, match="BayerPattern"):
        demosaic.directional(np.zeros((4, 4), f32), pattern=0)
    with pytest.raises(AssertionError):
        demosaic.directional(np.zeros((3, 4), f32))


def test_cli_argument():
    from taichi_image_amd.scripts import tonemap_scan
    ap = tonemap_scan.build_parser()
    assert ap.parse_args(["--images", "x"]).demosaic is None
    assert ap.parse_args(["--images", "x", "--demosaic", "directional"]).demosaic == "directional"
    assert ap.parse_args(["--images", "x", "--demosaic", "malvar"]).demosaic == "malvar"
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--demosaic", "menon"])
