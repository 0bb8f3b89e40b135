"""Highlight reconstruction without a GPU: the settings' validation (Python and the C entry points' host-side checks), the
properties of the contract on its NumPy restatement (tests/highlights_ref.py), one hand-computed vector, and the command
line's argument checks."""
import ctypes

import numpy as np
import pytest

from oracle import isp_oracle as O
from tests import highlights_ref as R

f32 = np.float32
WB = (1.8, 1.0, 2.1)
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]


@pytest.fixture(scope="module")
def hl():
    from taichi_image_amd import highlights
    return highlights


def ulps(a, b):
    a, b = f32(a), f32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_settings_validation(hl):
    h = hl.Highlights()
    assert (h.mode, h.clip) == ("rebuild", 0.98)
    assert hl.Highlights("clip", 0.9).mode == "clip"
    for bad in ("blend", "", None, 0, b"clip"):
        with pytest.raises(ValueError):
            hl.Highlights(mode=bad)
    for bad in (0, 0.0, -0.5, float("nan"), float("inf"), 1e39, 1e-50, "0.9", None, True):
        with pytest.raises(ValueError):
            hl.Highlights(clip=bad)
    assert hl.check_highlights(None) is None and hl.check_highlights(h) is h
    for bad in (True, "rebuild", 0.98, ("rebuild", 0.98)):
        with pytest.raises(ValueError):
            hl.check_highlights(bad)
    for bad in ((1, 1), (1, 0, 1), (1, -1, 1), (1, float("nan"), 1), (1, 1e39, 1), 3.0, ("a", 1, 1)):
        with pytest.raises(ValueError):
            hl.check_white_balance(bad)
    assert hl.check_white_balance(np.array([1.8, 1.0, 2.1])) == tuple(float(f32(v)) for v in WB)
    arg = h._arg(WB)
    assert arg.mode == 0 and f32(arg.clip) == f32(0.98) and arg.wb_dev is None
    assert [f32(v) for v in arg.wb] == [f32(v) for v in WB]
    with pytest.raises(ValueError):
        hl.reconstruct_cfa(np.zeros((4, 4), f32), O.RGGB)                      # (a BayerPattern, not its number)
    import taichi_image_amd as ti
    with pytest.raises(ValueError):
        hl.reconstruct_cfa(np.zeros((4, 4), f32), ti.BayerPattern.RGGB, highlights="rebuild")
    with pytest.raises(ValueError):
        hl.reconstruct_cfa(np.zeros((4, 4), np.uint16), ti.BayerPattern.RGGB)
    assert ti.Highlights is hl.Highlights


def test_c_entry_points_reject_bad_settings_before_any_launch():
    from taichi_image_amd import _native
    L = _native.lib()
    a, b = (ctypes.c_float * 16)(), (ctypes.c_float * 16)()
    pa, pb = ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p)

    def settings(mode=0, clip=0.98, wb=(1.0, 1.0, 1.0)):
        return _native.Highlights(mode, clip, (ctypes.c_float * 3)(*wb), None)

    def rejected(rc):
        assert rc != 0
        assert b"highlights" in L.mi_isp_last_error(), L.mi_isp_last_error()

    F32 = _native.MI_F32
    rejected(L.mi_isp_highlights_cfa(pa, pb, 4, 4, F32, 0, None, None))
    rejected(L.mi_isp_highlights_cfa(pa, pb, 4, 4, F32, 0, settings(mode=2), None))
    rejected(L.mi_isp_highlights_cfa(pa, pb, 4, 4, F32, 0, settings(mode=-1), None))
    for clip in (0.0, -1.0, float("nan"), float("inf")):
        rejected(L.mi_isp_highlights_cfa(pa, pb, 4, 4, F32, 0, settings(clip=clip), None))
    for wb in ((0.0, 1.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        rejected(L.mi_isp_highlights_cfa(pa, pb, 4, 4, F32, 0, settings(wb=wb), None))
    rejected(L.mi_isp_highlights_cfa(pa, pb, 4, 4, F32, 4, settings(), None))              # pattern
    rejected(L.mi_isp_highlights_cfa(pa, pb, 4, 4, _native.MI_U16, 0, settings(), None))   # dtype
    rejected(L.mi_isp_highlights_cfa(pa, pa, 4, 4, F32, 0, settings(), None))              # in place
    rejected(L.mi_isp_highlights_cfa(None, pb, 4, 4, F32, 0, settings(), None))
    rejected(L.mi_isp_highlights_cfa(pa, pb, -1, 4, F32, 0, settings(), None))
    raw = lambda **kw: L.mi_isp_highlights_raw(  # noqa: E731
        kw.get("src", pa), kw.get("dst", pb), kw.get("H", 4), kw.get("W", 4), kw.get("kind", _native.MI_RAW_32F),
        kw.get("ids", 0), kw.get("work", F32), kw.get("pattern", 0), kw.get("levels"), kw.get("shading"), None,
        kw.get("s", settings()), kw.get("plain", 0), None)
    rejected(raw(s=settings(clip=0.0)))
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
    batch = lambda n, H, W, s=None: L.mi_isp_highlights_raw_batch(  # noqa: E731
        one, out, n, H, W, _native.MI_RAW_32F, 0, F32, 0, None, None, None, s or settings(), 0, None)
    rejected(batch(-1, 4, 4))
    rejected(batch(0, 4, 4, settings(mode=9)))                                                # (checked even for no frames)
    # n == 0 and H * W == 0 are successful no-ops
    assert batch(0, 4, 4) == 0 and batch(1, 0, 4) == 0 and batch(1, 4, 0) == 0
    assert L.mi_isp_highlights_cfa(pa, pb, 0, 4, F32, 0, settings(), None) == 0
    assert raw(H=0) == 0


def test_isp_arguments_are_checked_without_a_device():
    """The constructor rejects a wrong highlights= before it touches the device."""
    import taichi_image_amd as ti
    with pytest.raises(ValueError, match="highlights"):
        ti.Camera16(ti.BayerPattern.RGGB, highlights="rebuild")
    with pytest.raises(ValueError, match="highlights"):
        ti.Camera32(ti.BayerPattern.RGGB, highlights=0.98)


# ---- the contract's properties on the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_no_clipped_pixel_is_the_identity(rng, pattern):
    x = (rng.random((34, 38)) * 0.97).astype(f32)
    assert x.max() < f32(0.98)
    y = R.reconstruct(x, pattern, WB)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("wb", [WB, (1.0, 1.0, 1.0), (2.5, 1.0, 1.3)])
def test_never_lowers_a_pixel(rng, pattern, wb):
    H, W = 66, 70
    codes = R.make_codes(rng, H, W, 4095, int(0.985 * 4095) + 1, pattern)
    x = codes.astype(f32) * f32(1 / 4095)
    y = R.reconstruct(x, pattern, wb)
    assert (y >= x).all()
    assert np.array_equal(y[x < f32(0.98)], x[x < f32(0.98)]), "only clipped pixels change"
    frac, kept = R.coverage(x, y, 0.98, H, W)
    assert frac >= 0.05 and min(kept) >= 1, (frac, kept)


@pytest.mark.parametrize("H,W", [(64, 64), (66, 70), (130, 66)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_generated_frames_exercise_the_operator(rng, H, W, pattern):
    """What the GPU cases assert on the reference: 5 % of the pixels raised, a clipped pixel per site left alone."""
    for wb in (WB, (1.0, 1.0, 1.0)):
        codes = R.make_codes(rng, H, W, 4095, int(0.985 * 4095) + 1, pattern)
        x = codes.astype(f32) * f32(1 / 4095)
        frac, kept = R.coverage(x, R.reconstruct(x, pattern, wb), 0.98, H, W)
        assert frac >= 0.05 and min(kept) >= 1, (wb, frac, kept)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("mode", ["rebuild", "clip"])
def test_a_blown_out_frame_comes_out_neutral(pattern, mode):
    H, W = 8, 10
    x = np.ones((H, W), f32)
    y = R.reconstruct(x, pattern, WB, mode, 0.98)
    bal = (y * R.gain_map(WB, pattern, H, W)).astype(f32)
    want = f32(max(WB)) if mode == "rebuild" else f32(f32(0.98) * f32(min(WB)))
    worst = max(ulps(v, want) for v in bal.ravel())
    assert worst <= 2, (worst, bal)
    if mode == "rebuild":
        assert (y >= x).all()
    else:
        assert (y <= x).all()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_saturated_pure_colour_is_left_alone(pattern):
    H, W = 12, 12
    x = np.full((H, W), 0.04, f32)
    red = np.asarray(R.COLOURS[pattern])[R.site_map(H, W)] == 0
    x[red] = 1.0                                                             # red clipped, green and blue dark
    y = R.reconstruct(x, pattern, WB)
    assert np.array_equal(y, x)


def test_a_lone_clipped_green_rises_to_its_brighter_neighbour_mean():
    x = np.full((6, 6), 0.2, f32)
    x[2, 3] = 1.0                                                            # RGGB: (2, 3) is a G site in an R row
    x[2, 2], x[2, 4] = 0.7, 0.8                                              # its R neighbours (w 1.8): mean b 1.35
    x[1, 3], x[3, 3] = 0.3, 0.5                                              # its B neighbours (w 2.1): mean b 0.84
    y = R.reconstruct(x, O.RGGB, WB)
    m = f32(f32(f32(0.7) * f32(1.8) + f32(0.8) * f32(1.8)) / f32(2))
    assert y[2, 3] == f32(m / f32(1.0)) and y[2, 3] > 1.3
    changed = y != x
    assert changed.sum() == 1 and changed[2, 3]


def test_a_listed_defect_feeds_no_estimate_and_a_centre_without_taps_is_unchanged():
    x = np.full((6, 6), 0.2, f32)
    x[2, 3] = 1.0
    x[2, 2], x[2, 4] = 0.9, 0.5                                              # (2, 2) would dominate ...
    mask = np.zeros((6, 6), bool)
    y_all = R.reconstruct(x, O.RGGB, WB, excluded=mask)
    mask[2, 2] = True                                                        # ... but is a listed defect
    y = R.reconstruct(x, O.RGGB, WB, excluded=mask)
    assert y_all[2, 3] == f32(f32(f32(0.9) * f32(1.8) + f32(0.5) * f32(1.8)) / f32(2))
    assert y[2, 3] == x[2, 3], "only (2, 4) is left in the group: b 0.9 < b(p) 1.0"
    x[2, 4] = 0.7
    assert R.reconstruct(x, O.RGGB, WB, excluded=mask)[2, 3] == f32(f32(0.7) * f32(1.8))     # n = 1: the tap itself
    for q in ((2, 2), (2, 4), (1, 3), (3, 3)):                               # every tap of the G site listed
        mask[q] = True
    x[1, 3] = x[3, 3] = 0.9
    assert R.reconstruct(x, O.RGGB, WB, excluded=mask)[2, 3] == x[2, 3]
    mask[...] = False
    mask[2, 3] = True                                                        # a listed centre keeps x, in both modes
    assert R.reconstruct(x, O.RGGB, WB, excluded=mask)[2, 3] == x[2, 3]
    assert R.reconstruct(x, O.RGGB, WB, "clip", 0.5, excluded=mask)[2, 3] == x[2, 3]


def test_corners_and_edges_use_the_taps_inside_the_frame():
    x = np.full((4, 6), 0.25, f32)
    x[0, 0] = 1.0                                                            # RGGB corner, an R site: taps (0, 1), (1, 0); (1, 1)
    x[0, 1], x[1, 0], x[1, 1] = 0.5, 0.7, 0.7
    y = R.reconstruct(x, O.RGGB, (1.0, 2.0, 1.5))
    mA = f32(f32(f32(0.5) * f32(2) + f32(0.7) * f32(2)) / f32(2))            # two of four G taps
    mB = f32(f32(0.7) * f32(1.5))                                            # one of four B taps
    assert mA > mB and y[0, 0] == f32(mA / f32(1.0))
    x = np.full((4, 6), 0.25, f32)
    x[3, 2] = 1.0                                                            # bottom edge, a G site in a B row: (3, 1), (3, 3); (2, 2)
    x[2, 2] = 0.9
    y = R.reconstruct(x, O.RGGB, (2.0, 1.0, 1.5))
    assert y[3, 2] == f32(f32(0.9) * f32(2.0))                               # the one column tap (R) alone: n = 1
    m, n = R._group_mean(np.ones((2, 2), f32), np.ones((2, 2), bool), R.RB_A)
    assert n.tolist() == [[2, 2], [2, 2]]
    m, n = R._group_mean(np.ones((2, 2), f32), np.ones((2, 2), bool), R.RB_B)
    assert n.tolist() == [[1, 1], [1, 1]]


def test_hand_computed_vector():
    """RGGB, w = (2, 1, 4), t = 0.75; every value is exact in binary, worked by hand (not by the reference):
    (0, 0) R, x = t: G taps (0,1), (1,0): b 0.5, 0.5 -> 0.5; B tap (1,1): 0.5 * 4 = 2 -> e = 2 > b = 1.5: y = 2 / 2 = 1
    (1, 2) G: row taps (1,1) 2.0, (1,3) 0.5 -> 1.25; column taps (0,2) 1.25, (2,2) 1.0 -> 1.125; e = 1.25 > 1: y = 1.25
    (2, 3) G on the right edge: row tap (2,2) 1.0 alone -> 1.0; column taps 0.5, 0.5 -> 0.5; e = 1.0 is not > b = 1.0: kept
    (3, 0) G in the corner: row tap (3,1) 0.5; column tap (2,0) 1.25; e = 1.25 > 1: y = 1.25"""
    x = np.array([[0.75, 0.5, 0.625, 0.5],
                  [0.5, 0.5, 1.0, 0.125],
                  [0.625, 0.5, 0.5, 1.0],
                  [1.0, 0.125, 0.5, 0.125]], f32)
    want = np.array([[1.0, 0.5, 0.625, 0.5],
                     [0.5, 0.5, 1.25, 0.125],
                     [0.625, 0.5, 0.5, 1.0],
                     [1.25, 0.125, 0.5, 0.125]], f32)
    assert np.array_equal(R.reconstruct(x, O.RGGB, (2.0, 1.0, 4.0), "rebuild", 0.75), want)
    # clip: t * min(w) = 0.75; the limits are 0.375 (R), 0.75 (G), 0.1875 (B)
    want_clip = np.array([[0.375, 0.5, 0.375, 0.5],
                          [0.5, 0.1875, 0.75, 0.125],
                          [0.375, 0.5, 0.375, 0.75],
                          [0.75, 0.125, 0.5, 0.125]], f32)
    assert np.array_equal(R.reconstruct(x, O.RGGB, (2.0, 1.0, 4.0), "clip", 0.75), want_clip)
    # t is compared with >=, and in f32: 0.75 is clipped at t = 0.75, not at the next f32 above it
    above = float(np.nextafter(f32(0.75), f32(1)))
    assert R.reconstruct(x, O.RGGB, (2.0, 1.0, 4.0), "rebuild", above)[0, 0] == f32(0.75)


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_cli_arguments(tmp_path):
    from taichi_image_amd.scripts import tonemap_scan
    ap = tonemap_scan.build_parser()
    a = ap.parse_args(["--images", "x"])
    assert a.highlights is None and a.highlights_clip is None
    a = ap.parse_args(["--images", "x", "--highlights", "clip", "--highlights-clip", "0.9"])
    assert a.highlights == "clip" and a.highlights_clip == 0.9
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--highlights", "blend"])
    missing = str(tmp_path / "no_such_scan")                                  # (never read: the checks come first)
    with pytest.raises(ValueError, match="--highlights-clip needs --highlights"):
        tonemap_scan.main(["--images", missing, "--highlights-clip", "0.9"])
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(ValueError, match="clip"):
            tonemap_scan.main(["--images", missing, "--highlights", "rebuild", "--highlights-clip", bad])
    with pytest.raises(FileNotFoundError):                                    # valid settings get as far as the scan
        tonemap_scan.main(["--images", missing, "--highlights", "rebuild", "--highlights-clip", "0.95"])
