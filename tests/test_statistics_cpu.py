"""The frame statistics reference (tests/statistics_ref.py) and the settings, without a GPU.

The reference is pinned by vectors worked out by hand from DESIGN.md 3, "Frame statistics"; it then has to satisfy the
contract's counting identities on random frames, its focus measure has to fall with defocus, and the inputs the GPU tests
generate have to exercise every rule - all checked on the reference alone."""
import ctypes

import numpy as np
import pytest

from oracle import isp_oracle as O
from tests import statistics_ref as R
from tests.test_demosaic_cpu import scenes

f32 = np.float32
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]


# ---- hand vectors ------------------------------------------------------------------------------------------------------
def test_a_2x2_frame():
    """One quad: one pixel per site, one zone, no focus pixel.  x = 0.5 -> v = 32768, bin 128; 1.0 -> 65536, bin 255, clipped;
    0 -> 0, bin 0, dark; 0.25 -> 16384, bin 64."""
    x = np.array([[0.5, 1.0], [0.0, 0.25]], f32)
    q = R.measure(x, O.RGGB, (1, 1), clip=0.98, dark=1 / 64)
    assert q.zones.tolist() == [[[[1, 32768, 0, 0], [1, 65536, 1, 0], [1, 0, 0, 1], [1, 16384, 0, 0]]]]
    assert q.focus.tolist() == [[[0, 0]]]
    assert [(int(s), int(k)) for s, k in zip(*np.nonzero(q.histogram))] == [(0, 128), (1, 255), (2, 0), (3, 64)]
    assert q.words.shape == (R.words((1, 1)),) and q.words.dtype == np.int64


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_6x6_frame_has_one_focus_pixel_per_green_phase(pattern):
    """Only rows and columns 2 and 3 have all four taps inside: the two green pixels among (2, 2), (2, 3), (3, 2), (3, 3).
    x = k / 64 with k = 6 r + c, so v = 1024 k; L = 4 v(p) - sum of the taps = 0 on this plane, and 1024 * 4 * 9 with the
    centre raised by 9 / 64."""
    k = np.arange(36).reshape(6, 6)
    x = (k / 64).astype(f32)
    gp = R.green_parity(pattern)
    centres = [(r, c) for r in (2, 3) for c in (2, 3) if ((r + c) & 1) == gp]
    q = R.measure(x, pattern, (1, 1))
    assert [tuple(p) for p in np.argwhere(q.contributes)] == centres and q.focus.tolist() == [[[0, 2]]]
    x[centres[0]] += f32(9 / 64)
    q = R.measure(x, pattern, (3, 3))
    assert q.focus[1, 1].tolist() == [(4 * 9 * 1024) ** 2, 2] and int(q.focus.sum()) == (4 * 9 * 1024) ** 2 + 2
    assert int(q.zones[1, 1, :, 1].sum()) == 1024 * (14 + 15 + 20 + 21 + 9)


def test_exactly_at_clip_and_at_dark():
    """x == f32(clip) is clipped (>=) and leaves the focus sum; the f32 below is not.  x == f32(dark) is dark (<=); the
    f32 above is not."""
    clip, dark = f32(0.7), f32(0.1)
    x = np.full((6, 6), 0.5, f32)
    x[2, 3], x[0, 0], x[0, 2] = clip, np.nextafter(clip, f32(0)), dark
    x[1, 1] = np.nextafter(dark, f32(1))
    q = R.measure(x, O.RGGB, (1, 1), clip=0.7, dark=0.1)
    assert q.clipped[2, 3] and int(q.clipped.sum()) == 1 and q.dark[0, 2] and int(q.dark.sum()) == 1
    assert [tuple(p) for p in np.argwhere(q.contributes)] == [(3, 2)]         # (2, 3) is clipped itself
    x[2, 3], x[3, 0] = 0.5, clip                                              # ... and now a tap of (3, 2) is
    q = R.measure(x, O.RGGB, (1, 1), clip=0.7, dark=0.1)
    assert [tuple(p) for p in np.argwhere(q.contributes)] == [(2, 3)] and q.tap_rejected[3, 2]


def test_rounding_ties_go_to_even():
    """x * 65536 is exact in f32; k + 0.5 rounds to the even neighbour."""
    x = np.zeros((2, 4), f32)
    x[0] = [0.5 / 65536, 1.5 / 65536, 2.5 / 65536, 3.5 / 65536]
    x[1] = [(255 * 256 + 255.5) / 65536, (255 * 256 + 254.5) / 65536, 0.75 / 65536, 0.25 / 65536]
    q = R.measure(x, O.RGGB, (1, 2))
    assert q.v.tolist() == [[0, 2, 2, 4], [65536, 65534, 1, 0]]
    assert q.histogram[2, 255] == 1 and q.histogram[3, 255] == 1


def test_a_nan_a_masked_centre_and_a_masked_tap():
    x = np.full((8, 8), 0.25, f32)
    x[4, 3] = 0.5                                                             # green under RGGB, taps inside: L = 4 * 16384
    base = R.measure(x, O.RGGB, (1, 1))
    n = int(base.focus[0, 0, 1])
    assert n == 8 and int(base.focus[0, 0, 0]) == 65536 ** 2 + 2 * 16384 ** 2  # (4, 3), and (2, 3), (4, 5) that have it as a tap
    nan = x.copy()
    nan[4, 3] = np.nan                                                        # no pixel, no centre and no tap
    q = R.measure(nan, O.RGGB, (1, 1))
    assert not q.valid[4, 3] and int(q.zones[0, 0, :, 0].sum()) == 63 and q.focus.tolist() == [[[0, n - 3]]]
    assert int(q.histogram.sum()) == 63
    mask = np.zeros((8, 8), bool)
    mask[4, 3] = True                                                         # a masked centre: the same
    assert np.array_equal(R.measure(x, O.RGGB, (1, 1), excluded=mask).words, q.words)
    mask[:] = False
    mask[4, 1] = True                                                         # a tap of (4, 3) alone (no centre: column 1)
    q = R.measure(x, O.RGGB, (1, 1), excluded=mask)
    assert q.focus.tolist() == [[[2 * 16384 ** 2, n - 1]]] and not q.contributes[4, 3] and not q.contributes[4, 1]
    for bad in (-np.inf, np.inf):
        inf = x.copy()
        inf[4, 3] = bad                                                       # -inf is no pixel; +inf is one, clipped, v = 65536
        q = R.measure(inf, O.RGGB, (1, 1))
        assert q.valid[4, 3] == (bad > 0) and q.clipped[4, 3] == (bad > 0) and q.focus[0, 0, 1] == n - 3


def test_zones_follow_the_quad_row():
    """H = 10, gh = 3: quads 0, 1 -> zone 0 (0 and 3 over 5), quads 2, 3 -> zone 1 (6 and 9), quad 4 -> zone 2."""
    q = R.measure(np.zeros((10, 14), f32), O.RGGB, (3, 5))
    assert q.zi[:, 0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]
    assert q.zj[0].tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4]


# ---- identities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_counting_identities(rng, pattern):
    H, W = 66, 70
    x = (R.make_frame(rng, H, W).astype(f32) * f32(1 / 4095))
    x[rng.random((H, W)) < 0.01] = np.nan
    mask = rng.random((H, W)) < 0.01
    q = R.measure(x, pattern, (3, 5), excluded=mask)
    valid = ~mask & ~np.isnan(x)
    r, c = np.mgrid[0:H, 0:W]
    per_site = [int((valid & ((r & 1) * 2 + (c & 1) == s)).sum()) for s in range(4)]
    assert q.zones[..., 0].sum(axis=(0, 1)).tolist() == per_site
    assert q.histogram.sum(axis=1).tolist() == per_site
    assert int(q.focus[..., 1].sum()) == int(q.contributes.sum()) > 0
    assert int(q.zones[..., 2].sum()) == int((valid & (x >= f32(0.98))).sum())
    assert int(q.focus[..., 0].sum()) == int((q.L.astype(object) ** 2).sum())


# ---- focus measures focus ------------------------------------------------------------------------------------------------
def box_blur(img, radius):
    if radius == 0:
        return img
    n = 2 * radius + 1
    p = np.pad(img.astype(np.float64), ((radius, radius), (radius, radius), (0, 0)), mode="edge")
    out = np.zeros(img.shape, np.float64)
    for dy in range(n):
        for dx in range(n):
            out += p[dy:dy + img.shape[0], dx:dx + img.shape[1]]
    return (out / (n * n)).astype(f32)


@pytest.mark.parametrize("name", ["zone plate", "bars"])
def test_focus_falls_with_defocus(name):
    """The scenes of tests/test_demosaic_cpu.py scaled by 0.9, box-blurred at radius 0 .. 3, mosaicked through the oracle,
    with Gaussian noise of sigma 0.005: the mean L^2 falls strictly with the radius (measured: zone plate 0.885, 0.252,
    0.033, 0.011; bars 0.646, 0.246, 0.057, 0.0009)."""
    rng = np.random.default_rng(7)
    img = scenes()[name] * f32(0.9)
    got = []
    for radius in range(4):
        cfa = O.rgb_to_bayer(box_blur(img, radius), O.RGGB).astype(np.float64)
        x = (cfa + rng.normal(0.0, 0.005, cfa.shape)).astype(f32)
        q = R.measure(x, O.RGGB, (1, 1))
        got.append(float(R.sharpness(q)[0, 0]))
    print(f"{name}: mean L^2 {got}")
    assert all(a > b for a, b in zip(got, got[1:])) and got[0] > 10 * got[3]


# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,zones", [((66, 70), (3, 5)), ((66, 66), (2, 2)), ((190, 134), (3, 4)), ((190, 134), (6, 32)),
                                         ((256, 2048), (8, 8)), ((256, 2048), (32, 28))])
def test_the_generated_frames_exercise_every_rule(rng, shape, zones):
    for top in (4095, 65535):
        x = R.make_frame(rng, *shape, top).astype(f32) / f32(top)
        R.assert_exercised(R.measure(x, O.RGGB, zones), f"{shape} {zones}")


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_settings_errors():
    from taichi_image_amd import Statistics, check_statistics
    s = Statistics()
    assert s.zones == (8, 8) and s.clip == 0.98 and s.dark == 1 / 64 and s.words == 8 * 8 * 18 + 1024
    assert Statistics(zones=[2, 32]).zones == (2, 32) and check_statistics(None) is None and check_statistics(s) is s
    for zones in [(0, 8), (8, 33), (8,), (8, 8, 8), 8, (8.0, 8), (True, 8), None, "88"]:
        with pytest.raises(ValueError, match="Statistics.zones must be two integers in 1 .. 32"):
            Statistics(zones=zones)
    for clip in [0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-46, "1", None, True]:
        with pytest.raises(ValueError, match="Statistics.clip must be"):
            Statistics(clip=clip)
    for dark in [-0.1, 0.98, 1.0, float("nan"), float("inf"), "0", None, False, 0.98 - 1e-12]:
        with pytest.raises(ValueError, match="Statistics.dark must be"):
            Statistics(dark=dark)
    assert Statistics(dark=0).dark == 0 and Statistics(clip=2, dark=1).clip == 2
    with pytest.raises(ValueError, match="statistics must be None or a Statistics"):
        check_statistics((8, 8))
    a = s._arg()
    assert (a.zones_h, a.zones_w, a.clip, a.dark) == (8, 8, f32(0.98), f32(1 / 64))


def test_camera_and_entry_arguments():
    from taichi_image_amd import BayerPattern, Statistics, statistics_cfa
    from taichi_image_amd.camera_isp import _OPTIONAL_STAGES
    assert "statistics" in [name for name, _, _ in _OPTIONAL_STAGES]
    with pytest.raises(ValueError, match="settings must be a Statistics"):
        statistics_cfa(np.zeros((4, 4), f32), BayerPattern.RGGB, (8, 8))
    with pytest.raises(ValueError, match="pattern must be a BayerPattern"):
        statistics_cfa(np.zeros((4, 4), f32), 0, Statistics())
    with pytest.raises(ValueError, match="takes an f16 or f32 CFA"):
        statistics_cfa(np.zeros((4, 4), np.uint16), BayerPattern.RGGB, Statistics())


def test_the_header_constants_and_the_route_query():
    """The host-only queries: the geometry the GPU tests are written with, the words per frame, and the blocks that add to
    global memory directly - none while the zones of a block fit its table, every block with pixels of more cells."""
    from taichi_image_amd import Statistics, _native as N
    L = N.lib()
    out = (ctypes.c_int32 * 4)()
    assert L.mi_isp_statistics_geometry(out) == 0 and tuple(out) == (64, 64, 16, 16)
    assert L.mi_isp_statistics_words(Statistics()._arg()) == 8 * 8 * 18 + 1024
    assert L.mi_isp_statistics_words(Statistics(zones=(32, 32))._arg()) == R.words((32, 32))
    assert L.mi_isp_statistics_words(N.Statistics(0, 8, 0.98, 0.01)) == -1 and L.mi_isp_statistics_words(None) == -1
    blocks = lambda n, H, W, z: L.mi_isp_statistics_direct_blocks(n, H, W, Statistics(zones=z)._arg())
    assert blocks(6, 3072, 4096, (8, 8)) == 0 and blocks(1, 10, 14, (3, 5)) == 0 and blocks(1, 10, 14, (5, 7)) == 1
    assert blocks(1, 66, 66, (32, 3)) == 2 and blocks(1, 190, 134, (6, 32)) == 6 and blocks(32, 256, 2048, (32, 28)) == 32
    assert blocks(1, 3072, 4096, (32, 32)) == 0 and blocks(1, 128, 128, (32, 32)) == 4 and blocks(0, 10, 14, (5, 7)) == 0
    # the tiles a block takes in one launch: about 2048 blocks, at most 16 tiles, the strips of a tile row of equal length
    strip = L.mi_isp_statistics_strip
    assert [strip(n, 3072, 4096) for n in (1, 6, 32)] == [1, 8, 16] and strip(6, 1440, 1920) == 2
    assert strip(32, 256, 2048) == 2 and strip(32, 1024, 4096) == 16 and strip(32, 64, 64 * 20) == 1 and strip(32, 4096, 64 * 20) == 10


def test_the_shape_rules_of_the_settings():
    """Statistics.check_shape: what the loaders check before anything is uploaded or launched."""
    from taichi_image_amd import Statistics
    s = Statistics(zones=(3, 5))
    for shape in [(6, 10), (66, 70), (0, 7), (5, 0), (8192, 8192)]:
        s.check_shape(shape)
    for shape, text in [((5, 10), "statistics: frames must be even size, got 5x10"),
                        ((6, 11), "statistics: frames must be even size, got 6x11"),
                        ((4, 10), "statistics: zones 3x5 exceed the 2x5 quads of the frame"),
                        ((6, 8), "statistics: zones 3x5 exceed the 3x4 quads of the frame"),
                        ((8194, 8192), "statistics: frame 8194x8192 is too large"),
                        (((1 << 22) - 2, 10), "is too large")]:
        with pytest.raises(ValueError, match=text):
            s.check_shape(shape)
