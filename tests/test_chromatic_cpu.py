"""Chromatic aberration correction without a GPU: the settings' validation (Python and the C entry points' host-side
checks, the shift limit among them), the properties of the contract on its NumPy restatement (tests/chromatic_ref.py),
one hand-computed vector, and the command line's argument checks."""
import ctypes
import math

import numpy as np
import pytest

from oracle import isp_oracle as O
from tests import chromatic_ref as R

f32 = np.float32
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]
SHAPES = [(64, 64), (66, 70), (130, 66), (65, 67)]


@pytest.fixture(scope="module")
def ca():
    from taichi_image_amd import chromatic
    return chromatic


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_settings_validation(ca):
    import taichi_image_amd as ti
    s = ca.ChromaticAberration()
    assert (s.red, s.blue, s.center, s.norm_radius) == ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0), None, None)
    assert ti.ChromaticAberration is ca.ChromaticAberration
    s = ca.ChromaticAberration([1.001, 0, 0], np.array([0.999, 1e-3, 0]), center=(10, 20.5), norm_radius=100)
    assert s.red == (1.001, 0.0, 0.0) and s.center == (10.0, 20.5) and s.norm_radius == 100.0
    for bad in ((1, 0), (1, 0, 0, 0), 1.0, None, (1, float("nan"), 0), (1, 0, float("inf")), (1, 1e39, 0), ("1", 0, 0),
                (True, 0, 0)):
        with pytest.raises(ValueError):
            ca.ChromaticAberration(red=bad)
        with pytest.raises(ValueError):
            ca.ChromaticAberration(blue=bad)
    for bad in ((1,), (1, 2, 3), 5.0, (float("nan"), 0), (0, float("inf")), ("a", 0)):
        with pytest.raises(ValueError):
            ca.ChromaticAberration(center=bad)
    for bad in (0, 0.0, -3.0, float("nan"), float("inf"), 1e-30, "7", True):
        with pytest.raises(ValueError):
            ca.ChromaticAberration(norm_radius=bad)
    assert ca.check_chromatic_aberration(None) is None and ca.check_chromatic_aberration(s) is s
    for bad in (True, (1, 0, 0), 1.0, "on"):
        with pytest.raises(ValueError):
            ca.check_chromatic_aberration(bad)
    # the defaults of a frame: the middle of the frame, the half diagonal
    arg = ca.ChromaticAberration((1.25, 0.5, -0.5), (0.75, 0, 1))._arg((6, 8))
    assert (arg.cy, arg.cx, arg.norm_radius) == (2.5, 3.5, 5.0)
    assert list(arg.red) == [1.25, 0.5, -0.5] and list(arg.blue) == [0.75, 0.0, 1.0]
    arg = s._arg((6, 8))
    assert (arg.cy, arg.cx, arg.norm_radius) == (10.0, 20.5, 100.0)
    with pytest.raises(ValueError):
        ca.correct_cfa(np.zeros((4, 4), f32), O.RGGB, s)                       # (a BayerPattern, not its number)
    with pytest.raises(ValueError):
        ca.correct_cfa(np.zeros((4, 4), f32), ti.BayerPattern.RGGB, (1, 0, 0))
    with pytest.raises(ValueError):
        ca.correct_cfa(np.zeros((4, 4), np.uint16), ti.BayerPattern.RGGB, s)
    with pytest.raises(ValueError):
        ca.correct_cfa(np.zeros((4, 4, 1), f32), ti.BayerPattern.RGGB, s)


def test_the_shift_limit(ca):
    """|(k0 - 1) + q (k1 + q k2)| r at 1025 radii up to the farthest corner: 8.0 px passes, just over 8 px raises."""
    import taichi_image_amd as ti
    # centre (0, 0) on a 1 x 33 frame: the farthest corner is 32 px away, k0 - 1 = 0.25 gives 8.0 exactly
    at = ca.ChromaticAberration((1.25, 0, 0), (0.75, 0, 0), center=(0, 0), norm_radius=10)
    assert at.max_shift((1, 33)) == (8.0, 8.0)
    at.check_shape((1, 33))
    over = float(np.nextafter(1.25, 2.0))
    for s in (ca.ChromaticAberration((over, 0, 0), center=(0, 0), norm_radius=10),
              ca.ChromaticAberration(blue=(2.0 - over, 0, 0), center=(0, 0), norm_radius=10)):
        assert max(s.max_shift((1, 33))) > 8.0
        with pytest.raises(ValueError, match="chromatic"):
            s.check_shape((1, 33))
        with pytest.raises(ValueError, match="chromatic"):                       # before anything is uploaded
            ca.correct_cfa(np.zeros((1, 33), f32), ti.BayerPattern.RGGB, s)
    at.check_shape((0, 8))                                                       # (an empty frame has no shift)
    # the polynomial's terms: q = 1 at the corner with norm_radius = r; the maximum may lie inside the frame
    s = ca.ChromaticAberration((1, 0.125, 0.125), (1, 0.5, -0.5), center=(0, 0), norm_radius=32)
    red, blue = s.max_shift((1, 33))
    assert red == 8.0                                                            # (0.125 + 0.125) * 32 at the corner
    qs = (np.arange(1025) / 1024.0) ** 2
    assert blue == max(abs(q * (0.5 + q * -0.5)) * (32 * i / 1024.0) for i, q in enumerate(qs)) and 0 < blue < 8
    # the defaults: the middle of the frame, the half diagonal
    Rn = math.hypot(64, 96)
    s = ca.ChromaticAberration((1 + 3 / Rn, 2 / Rn, 0), (1 - 2.5 / Rn, -1 / Rn, 0))
    red, blue = s.max_shift((128, 192))
    assert 4.8 < red < 5.0 and 3.3 < blue < 3.5
    # the generated-frame settings of the GPU cases
    for H, W in SHAPES:
        k = R.frame_settings(H, W)
        red, blue = ca.ChromaticAberration(k.red, k.blue).max_shift((H, W))
        assert 5.6 <= red <= 5.9 and 4.7 <= blue <= 5.0, (H, W, red, blue)


def test_c_entry_points_reject_bad_settings_before_any_launch():
    from taichi_image_amd import _native
    L = _native.lib()
    a, b = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    pa, pb = ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p)
    D3 = ctypes.c_double * 3

    def settings(cy=1.5, cx=1.5, nr=4.0, red=(1.0, 0.0, 0.0), blue=(1.0, 0.0, 0.0)):
        return _native.Chromatic(cy, cx, nr, D3(*red), D3(*blue))

    def rejected(rc):
        assert rc != 0
        assert b"chromatic" in L.mi_isp_last_error(), L.mi_isp_last_error()

    F32 = _native.MI_F32
    nan, inf = float("nan"), float("inf")
    rejected(L.mi_isp_chromatic_cfa(pa, pb, 4, 4, F32, 0, None, None))
    for bad in (dict(cy=nan), dict(cx=inf), dict(nr=nan), dict(nr=inf), dict(nr=0.0), dict(nr=-4.0), dict(nr=1e-30),
                dict(red=(nan, 0, 0)), dict(red=(1, inf, 0)), dict(blue=(1, 0, nan)), dict(blue=(1e39, 0, 0)),
                dict(cy=1e39)):
        rejected(L.mi_isp_chromatic_cfa(pa, pb, 4, 4, F32, 0, settings(**bad), None))
    # the shift limit: centre (0, 0) on a 1 x 33 frame, 32 px to the farthest corner
    over = float(np.nextafter(1.25, 2.0))
    assert L.mi_isp_chromatic_cfa(pa, pb, 0, 33, F32, 0, settings(0, 0, 10, red=(over, 0, 0)), None) == 0    # (empty)
    rejected(L.mi_isp_chromatic_cfa(pa, pb, 1, 33, F32, 0, settings(0, 0, 10, red=(over, 0, 0)), None))
    rejected(L.mi_isp_chromatic_cfa(pa, pb, 1, 33, F32, 0, settings(0, 0, 10, blue=(2 - over, 0, 0)), None))
    rejected(L.mi_isp_chromatic_cfa(pa, pb, 1, 33, F32, 0, settings(0, 0, 32, blue=(1, 0.125, 0.126)), None))
    rejected(L.mi_isp_chromatic_cfa(pa, pb, 4, 4, F32, 4, settings(), None))              # pattern
    rejected(L.mi_isp_chromatic_cfa(pa, pb, 4, 4, _native.MI_U16, 0, settings(), None))   # dtype
    rejected(L.mi_isp_chromatic_cfa(pa, pa, 4, 4, F32, 0, settings(), None))              # in place
    rejected(L.mi_isp_chromatic_cfa(None, pb, 4, 4, F32, 0, settings(), None))
    rejected(L.mi_isp_chromatic_cfa(pa, pb, -1, 4, F32, 0, settings(), None))
    raw = lambda **kw: L.mi_isp_chromatic_raw(  # noqa: E731
        kw.get("src", pa), kw.get("dst", pb), kw.get("H", 4), kw.get("W", 4), kw.get("kind", _native.MI_RAW_32F),
        kw.get("ids", 0), kw.get("work", F32), kw.get("pattern", 0), kw.get("levels"), kw.get("shading"), None,
        kw.get("s", settings()), kw.get("plain", 0), None)
    rejected(raw(s=settings(nr=0.0)))
    rejected(raw(s=settings(red=(5.0, 0, 0))))                                                # 4 * 2.12 px on 4 x 4
    assert raw(H=0, s=settings(red=(5.0, 0, 0))) == 0
    rejected(raw(s=None))
    rejected(raw(kind=7))
    rejected(raw(pattern=-1))
    rejected(raw(src=None))
    rejected(raw(dst=pa))
    rejected(raw(kind=_native.MI_RAW_PACKED12, H=3))                                          # packed: even sizes
    rejected(raw(ids=1))                                                                      # IDS is a packed-12 layout
    rejected(raw(levels=_native.levels_arg([0, 0, 0, 0], 4095)))                              # levels: u16 codes only
    grid = _native.Shading(pa, 1, 2, 2)
    rejected(raw(shading=grid, plain=1))                                                      # plain y takes no grid
    one = (ctypes.c_void_p * 1)(pa)
    out = (ctypes.c_void_p * 1)(pb)
    batch = lambda n, H, W, s=None: L.mi_isp_chromatic_raw_batch(  # noqa: E731
        one, out, n, H, W, _native.MI_RAW_32F, 0, F32, 0, None, None, None, s or settings(), 0, None)
    rejected(batch(-1, 4, 4))
    rejected(batch(0, 4, 4, settings(nr=-1.0)))                                               # (checked even for no frames)
    rejected(batch(0, 1, 33, settings(0, 0, 10, red=(over, 0, 0))))
    # n == 0 and H * W == 0 are successful no-ops
    assert batch(0, 4, 4) == 0 and batch(1, 0, 4) == 0 and batch(1, 4, 0) == 0
    assert L.mi_isp_chromatic_cfa(pa, pb, 0, 4, F32, 0, settings(), None) == 0
    assert raw(H=0) == 0


def test_isp_arguments_are_checked_without_a_device():
    """The constructor rejects a wrong chromatic_aberration= before it touches the device."""
    import taichi_image_amd as ti
    with pytest.raises(ValueError, match="chromatic_aberration"):
        ti.Camera16(ti.BayerPattern.RGGB, chromatic_aberration=(1, 0, 0))
    with pytest.raises(ValueError, match="chromatic_aberration"):
        ti.Camera32(ti.BayerPattern.RGGB, chromatic_aberration=True)


# ---- the contract's properties on the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_identity_coefficients_are_the_identity(rng, pattern):
    """k = (1, 0, 0): e == 0, the displacement form gives vs == r exactly, so fr == fc == 0 and y = x * 1 + x' * 0."""
    x = rng.random((34, 39)).astype(f32)
    x[3, 4] = x[10, 11] = 0.0
    s = R.Settings(center=(11.3, 17.77), norm_radius=23.9)
    assert same_bits(R.correct(x, pattern, s), x)
    assert same_bits(R.correct(x, pattern, R.Settings()), x)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_green_sites_never_change(rng, pattern):
    H, W = 66, 70
    x = rng.random((H, W)).astype(f32)
    y = R.correct(x, pattern, R.frame_settings(H, W))
    rb = R.red_blue(pattern, H, W)
    assert same_bits(y[~rb], x[~rb])
    assert (y != x)[rb].mean() > 0.99
    mask = rng.random((H, W)) < 0.05                                         # (listed green sites keep x too)
    assert same_bits(R.correct(x, pattern, R.frame_settings(H, W), mask)[~rb], x[~rb])


def test_hand_computed_vector():
    """A 6 x 8 RGGB frame, centre (0, 0), norm_radius 8 (iR2 = 1 / 64), red (1.5, 0, 0), blue (0.5, 4, 0); every value is
    exact in binary, worked by hand (not by the reference).
    red (2, 2): e = 0.5, vs = us = 3: a = b = 1.5 -> cells (1, 1), (1, 2), (2, 1), (2, 2), fr = fc = 0.5
      = pixels (2, 2) 8, (2, 4) 16, (4, 2) 24, (4, 4) 32: mix(12, 28, 0.5) = 20
    red (4, 6): e = 0.5, vs = 6, us = 9: a = 3, b = 4.5 -> rows 3, 4 clamp to 2; columns 4, 5 clamp to 3: pixel (4, 6) = 40
    red (0, 2): vs = 0, us = 3: a = 0, b = 1.5: fr = 0: mix(mix(2, 4, 0.5), ., 0) = 3
    blue (1, 1): q = 2 / 64, e = -0.5 + 4 / 32 = -0.375, vs = us = 1 - 0.375 = 0.625: a = b = -0.1875: i = j = -1,
      fr = fc = 0.8125; rows -1, 0 clamp to 0, 0: the blue cell (0, 0) = pixel (1, 1) = 64 with every weight: 64
    blue (3, 1): dy = 3, dx = 1, q = 10 / 64, e = -0.5 + 0.625 = 0.125: vs = 3.375, us = 1.125: a = 1.1875, b = 0.0625
      -> rows 1, 2 (pixels 3, 5), columns 0, 1 (pixels 1, 3), fr = 0.1875, fc = 0.0625
      P = 128, 144 / 160, 176: mix over columns 129, 161; over rows 129 * 0.8125 + 161 * 0.1875 = 135"""
    x = np.zeros((6, 8), f32)
    x[0, 2], x[0, 4] = 2, 4
    x[2, 2], x[2, 4], x[4, 2], x[4, 4], x[4, 6] = 8, 16, 24, 32, 40
    x[1, 1] = 64
    x[3, 1], x[3, 3], x[5, 1], x[5, 3] = 128, 144, 160, 176
    s = R.Settings((1.5, 0, 0), (0.5, 4, 0), (0, 0), 8)
    y = R.correct(x, O.RGGB, s)
    assert y[2, 2] == 20 and y[4, 6] == 40 and y[0, 2] == 3 and y[1, 1] == 64 and y[3, 1] == 135
    # the same pixels under BGGR with the channels' coefficients swapped
    assert R.correct(x, O.BGGR, R.Settings(s.blue, s.red, (0, 0), 8))[3, 1] == 135


def test_a_masked_tap_feeds_nothing():
    x = np.zeros((6, 8), f32)
    x[2, 2], x[2, 4], x[4, 2], x[4, 4] = 8, 16, 24, 32
    s = R.Settings((1.5, 0, 0), (1, 0, 0), (0, 0), 8)                         # red (2, 2): four taps of weight 0.25
    mask = np.zeros((6, 8), bool)
    mask[2, 4] = True
    y = R.correct(x, O.RGGB, s, mask)
    assert y[2, 2] == f32(f32(f32(0.25 * 8) + f32(0.25 * 24) + f32(0.25 * 32)) / f32(0.75))
    x2 = x.copy()
    x2[2, 4] = 1e6                                                            # its value does not matter
    assert same_bits(R.correct(x2, O.RGGB, s, mask)[2, 2], y[2, 2])
    assert R.correct(x2, O.RGGB, s)[2, 2] != y[2, 2]
    mask[2, 2] = True                                                         # the pixel itself listed: a tap like any other
    assert R.correct(x, O.RGGB, s, mask)[2, 2] == f32(f32(f32(0.25 * 24) + f32(0.25 * 32)) / f32(0.5))
    # a kept tap of weight 0 only: S = 0, y = x(p)
    s0 = R.Settings((1.5, 0, 0), (1, 0, 0), (0, 2), 8)                        # red (2, 2): dx = 0: us = 2, fc = 0; vs = 3
    mask[...] = False
    mask[2, 2] = mask[4, 2] = True                                            # the column-0 taps listed, column 1 has w = 0
    assert R.correct(x, O.RGGB, s0, mask)[2, 2] == x[2, 2]


def test_all_four_taps_masked_gives_x():
    x = np.zeros((6, 8), f32)
    x[2, 2], x[2, 4], x[4, 2], x[4, 4] = 8, 16, 24, 32
    s = R.Settings((1.5, 0, 0), (1, 0, 0), (0, 0), 8)
    mask = np.zeros((6, 8), bool)
    for p in ((2, 2), (2, 4), (4, 2), (4, 4)):
        mask[p] = True
    assert R.correct(x, O.RGGB, s, mask)[2, 2] == 8
    s = R.Settings((2.0, 0, 0), (1, 0, 0), (0, 0), 8)                         # red (2, 2) samples (4, 4) alone
    assert R.correct(x, O.RGGB, s)[2, 2] == 32
    assert R.correct(x, O.RGGB, s, mask)[2, 2] == 8


def test_realignment():
    """A scene whose red and blue planes are displaced by the inverse of the settings' scales comes back aligned: the
    mean absolute error of the red and blue sites against the aligned scene falls to a quarter or less."""
    H, W = 128, 192
    Rn = math.hypot(H / 2, W / 2)
    s = R.Settings((1 + 3 / Rn, 2 / Rn, 0), (1 - 2.5 / Rn, -1 / Rn, 0))
    cy, cx = (H - 1) / 2, (W - 1) / 2

    def scene(v, u):
        return 0.5 + 0.25 * np.sin(0.35 * u + 0.2 * v) + 0.2 * np.cos(0.3 * v - 0.1 * u)

    def inverse(k, v, u):
        """The position whose image under p -> centre + s(q(p)) (p - centre) is (v, u), by fixed-point iteration."""
        pv, pu = v.copy(), u.copy()
        for _ in range(60):
            q = ((pv - cy) ** 2 + (pu - cx) ** 2) / Rn ** 2
            sc = k[0] + k[1] * q + k[2] * q * q
            pv, pu = cy + (v - cy) / sc, cx + (u - cx) / sc
        return pv, pu

    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    aligned = scene(v, u)
    x = aligned.copy()
    colour = np.asarray(R.COLOURS[O.RGGB])[(np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)]
    for ch, k in ((0, s.red), (2, s.blue)):
        pv, pu = inverse(k, v, u)
        x[colour == ch] = scene(pv, pu)[colour == ch]
    x = x.astype(f32)
    y = R.correct(x, O.RGGB, s)
    for ch in (0, 2):
        before = np.abs(x - aligned)[colour == ch].mean()
        after = np.abs(y - aligned)[colour == ch].mean()
        assert after <= 0.25 * before, (ch, before, after)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_generated_frames_exercise_the_operator(rng, H, W, pattern):
    """What the GPU cases assert on the reference: half of the red / blue pixels sample another cell, 4 % have a clamped
    tap, and on random data every one changes that can: all but the pixels whose taps of non-zero weight are all their own
    cell (the four corner cells, and on odd-sized frames the centre and the edge pixels on its axes: at most 9 of the
    2048 or more red / blue pixels of these frames, under half a percent)."""
    x = rng.random((H, W)).astype(f32)
    moved, clamped, changed, fixed = R.coverage(x, pattern, R.frame_settings(H, W))
    assert moved >= 0.5 and clamped >= 0.04 and changed == 1.0 and fixed < 0.005, (moved, clamped, changed, fixed)


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_cli_arguments(tmp_path):
    from taichi_image_amd.scripts import tonemap_scan
    ap = tonemap_scan.build_parser()
    a = ap.parse_args(["--images", "x"])
    assert a.chromatic_aberration is None and a.chromatic_center is None and a.chromatic_norm_radius is None
    a = ap.parse_args(["--images", "x", "--chromatic-aberration", "1.001", "0", "0", "0.999", "1e-3", "0",
                       "--chromatic-center", "1500", "2000.5", "--chromatic-norm-radius", "2560"])
    assert a.chromatic_aberration == [1.001, 0, 0, 0.999, 1e-3, 0]
    assert a.chromatic_center == [1500, 2000.5] and a.chromatic_norm_radius == 2560
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--chromatic-aberration", "1", "0", "0"])
    missing = str(tmp_path / "no_such_scan")                                  # (never read: the checks come first)
    with pytest.raises(ValueError, match="need --chromatic-aberration"):
        tonemap_scan.main(["--images", missing, "--chromatic-center", "1", "2"])
    with pytest.raises(ValueError, match="need --chromatic-aberration"):
        tonemap_scan.main(["--images", missing, "--chromatic-norm-radius", "100"])
    ok = ["--chromatic-aberration", "1.001", "0", "0", "0.999", "0", "0"]
    for bad in (["--chromatic-norm-radius", "0"], ["--chromatic-norm-radius", "nan"], ["--chromatic-center", "inf", "0"]):
        with pytest.raises(ValueError, match="ChromaticAberration"):
            tonemap_scan.main(["--images", missing] + ok + bad)
    with pytest.raises(ValueError, match="ChromaticAberration"):
        tonemap_scan.main(["--images", missing, "--chromatic-aberration", "nan", "0", "0", "1", "0", "0"])
    with pytest.raises(FileNotFoundError):                                    # valid settings get as far as the scan
        tonemap_scan.main(["--images", missing] + ok + ["--chromatic-norm-radius", "2560"])
