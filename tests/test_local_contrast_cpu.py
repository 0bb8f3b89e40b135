"""Local contrast without a GPU: the NumPy statement of the contract (tests/local_contrast_ref.py) pinned by hand and by its
properties, the settings' checks in Python and in the C entry points, and the scan CLI's argument checks."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest

from taichi_image_amd import camera_isp
from taichi_image_amd import local_contrast as lcm
from taichi_image_amd.local_contrast import LocalContrast, check_local_contrast
from tests import local_contrast_ref as R
from tests.sharpen_ref import luma, scene_u8

SHAPES = [((1, 1), (1, 1)), ((16, 16), (16, 16)), ((37, 53), (3, 4)), ((70, 260), (2, 3)), ((130, 140), (8, 8)),
          ((300, 300), (1, 1)), ((400, 520), (2, 2))]


def grey(a):
    """An (H, W, 3) grey image of the (H, W) values a (R = G = B = v has luma v: 77 + 150 + 29 = 256)."""
    return np.repeat(np.asarray(a, np.uint8)[..., None], 3, axis=2)


# ---- the restatement, pinned by hand -----------------------------------------------------------------------------------
def test_two_by_two_one_tile_by_hand():
    """L = (10, 10 / 200, 50), one tile, n = 4, no clip: cdf = 2 from 10, 3 from 50, 4 from 200, so lut = (510 cdf + 4) // 8
    = 128, 191, 255.  One tile: a == b on both axes, E = lut[L].  strength 0.5 (S = 32): delta = ((E - L) 32 + 32) >> 6 =
    (118 + 1) >> 1 = 59, (55 + 1) >> 1 = 28, (141 + 1) >> 1 = 71.
    clip 2 (C = 512): c = max(1, 2048 >> 16) = 1, e = 1, the bin of 10 drops to 1, e >> 8 = 0, r = 1: s = 256, h[0] += 1:
    cdf = 1 from 0, 2 from 10, 3 from 50, 4 from 200; lut[0] = 514 // 8 = 64."""
    img = grey([[10, 10], [200, 50]])
    assert R.clahe_rgb(img, (1, 1), None, 1.0)[..., 0].tolist() == [[128, 128], [255, 191]]
    assert R.clahe_rgb(img, (1, 1), None, 0.5)[..., 1].tolist() == [[69, 69], [228, 121]]
    assert R.clahe_rgb(img, (1, 1), 2.0, 1.0)[..., 2].tolist() == [[128, 128], [255, 191]]
    lut = R.luts(luma(img), (1, 1), 2.0)[0, 0]
    assert lut[[0, 9, 10, 49, 50, 199, 200, 255]].tolist() == [64, 64, 128, 128, 191, 191, 255, 255]
    assert R.luts(luma(img), (1, 1), None)[0, 0][[0, 9, 10]].tolist() == [0, 0, 128]


def test_negative_deltas_floor_by_hand():
    """L = (200, 210 / 220, 230), one tile, no clip: lut = 64, 128, 191, 255, E - L = -136, -82, -29, 25.  S = 32:
    (-4352 + 32) >> 6 = floor(-67.5) = -68 (truncation: -67), (-2624 + 32) >> 6 = floor(-40.5) = -41 (truncation: -40),
    (-928 + 32) >> 6 = -14, (800 + 32) >> 6 = 13."""
    img = grey([[200, 210], [220, 230]])
    assert R.clahe_rgb(img, (1, 1), None, 0.5)[..., 0].tolist() == [[132, 169], [206, 243]]
    assert R.clahe_rgb(img, (1, 1), None, 0.5, truncate=True)[..., 0].tolist() == [[133, 170], [206, 243]]
    yuv = np.concatenate([img[..., 0], np.full((1, 2), 77, np.uint8)])
    assert R.clahe_yuv420(yuv, (1, 1), None, 0.5).tolist() == [[132, 169], [206, 243], [77, 77]]


def test_four_by_four_two_by_two_tiles_by_hand():
    """Flat 2 x 2 tiles 100 | 150 over 50 | 200, no clip: lut_t[v] = 255 from the tile's value on, else 0.  An axis of 4 in
    2 tiles: N = -2, 2, 6, 10, i0 = -1, 0, 0, 1, rem = 6, 2, 6, 2, w = 192, 64, 192, 64, (a, b) = (0, 0), (0, 1), (0, 1),
    (1, 1).  Pixel (0, 0): a == b both ways, E = lut_00[100] = 255.  Pixel (1, 1), L = 100, wy = wx = 64: l00 = 255, l01 =
    0 (150 > 100), l10 = 255 (50 <= 100), l11 = 0: top = bot = 192 * 255 = 48960, E = (256 * 48960 + 32768) >> 16 = 191.
    Pixel (1, 2), L = 150, wy = 64, wx = 192: l00 = l01 = l10 = 255, l11 = 0: top = 65280, bot = 64 * 255 = 16320, E =
    (192 * 65280 + 64 * 16320 + 32768) >> 16 = 13611008 >> 16 = 207."""
    L = np.zeros((4, 4), np.uint8)
    L[:2, :2], L[:2, 2:], L[2:, :2], L[2:, 2:] = 100, 150, 50, 200
    a, b, w = R.axis_weights(4, 2)
    assert (a.tolist(), b.tolist(), w.tolist()) == ([0, 0, 0, 1], [0, 1, 1, 1], [192, 64, 192, 64])
    want = [[255, 191, 255, 255], [255, 191, 207, 191], [191, 143, 255, 255], [255, 191, 255, 255]]
    assert R.clahe_rgb(grey(L), (2, 2), None, 1.0)[..., 0].tolist() == want
    assert R.equalised(L, (2, 2), None).tolist() == want


def test_residual_distribution_by_hand():
    """n = 1024 at clip 2: c = (512 * 1024) >> 16 = 8.  e = 3: nothing for every bin, one count each to bins 0, 85, 170
    (s = 256 // 3).  e = 300: one count for every bin (300 >> 8), r = 44, s = 5: one more to bins 0, 5, ..., 215."""
    h = np.zeros(256, np.int64)
    h[7], h[100:226], h[226] = 11, 8, 5
    assert h.sum() == 1024
    out = R.redistribute(h, 512, 1024)
    want = np.minimum(h, 8)
    want[[0, 85, 170]] += 1
    assert out.tolist() == want.tolist() and out.sum() == 1024
    h = np.zeros(256, np.int64)
    h[7], h[100:189], h[189] = 308, 8, 4
    assert h.sum() == 1024
    out = R.redistribute(h, 512, 1024)
    want = np.minimum(h, 8) + 1
    want[np.arange(44) * 5] += 1
    assert out.tolist() == want.tolist() and out.sum() == 1024
    assert R.redistribute(h, 0, 1024).tolist() == h.tolist()       # C == 0: no clip
    # r > 128: stride 1, the first r bins
    h = np.zeros(256, np.int64)
    h[3] = 1024
    out = R.redistribute(h, 512, 1024)                              # e = 1016: 3 for every bin, r = 248
    assert out[:248].tolist() == [4] * 3 + [12] + [4] * 244 and out[248:].tolist() == [3] * 8


# ---- the restatement's properties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,tiles", SHAPES)
def test_properties_on_the_scene(rng, shape, tiles):
    H, W = shape
    img = scene_u8(rng, H, W)
    L = luma(img)
    hist, n = R.histograms(L, tiles)
    assert int(n.sum()) == H * W and int(n.min()) >= 1
    for clip in (None, 1.0, 2.0, 4.0, 64.0):
        lut = R.luts(L, tiles, clip)
        assert lut.min() >= 0 and lut.max() <= 255 and (lut[..., 255] == 255).all()
        assert (np.diff(lut, axis=-1) >= 0).all()
        for i in range(tiles[0]):
            for j in range(tiles[1]):
                assert R.redistribute(hist[i, j], R.clip_q8(clip), int(n[i, j])).sum() == n[i, j]
        E = R.equalised(L, tiles, clip)
        assert E.min() >= 0 and E.max() <= 255
        assert np.array_equal(R.clahe_rgb(img, tiles, clip, 0.0), img)              # S = 0: the identity
    if H % 2 == 0 and W % 2 == 0:
        yuv = np.concatenate([L.astype(np.uint8), np.full((H // 2, W), 9, np.uint8)])
        assert np.array_equal(R.clahe_yuv420(yuv, tiles, 2.0, 0.0), yuv)
        assert np.array_equal(R.clahe_yuv420(yuv, tiles, 2.0)[H:], yuv[H:])


def test_a_pixel_at_a_tile_centre_sees_one_lut(rng):
    """Tiles of 5 x 7 pixels: the centre pixel of tile (i, j) has wy = wx = 0 and (ay, ax) = (i, j)."""
    H, W, tiles = 15, 28, (3, 4)
    ay, _, wy = R.axis_weights(H, tiles[0])
    ax, _, wx = R.axis_weights(W, tiles[1])
    L = luma(scene_u8(rng, H, W))
    lut, E = R.luts(L, tiles, 2.0), R.equalised(L, tiles, 2.0)
    for i in range(3):
        for j in range(4):
            y, x = 5 * i + 2, 7 * j + 3
            assert (ay[y], wy[y], ax[x], wx[x]) == (i, 0, j, 0)
            assert E[y, x] == lut[i, j, L[y, x]]
    # above the first row of centres and left of the first column a == b
    a, b, _ = R.axis_weights(H, tiles[0])
    assert a[:2].tolist() == b[:2].tolist() == [0, 0] and a[-2:].tolist() == b[-2:].tolist() == [2, 2]


def test_flat_image():
    """CLAHE's known behaviour: a flat 100 goes to 102 at clip 2 and to 255 without a clip."""
    img = np.full((300, 300, 3), 100, np.uint8)
    assert (R.clahe_rgb(img, (1, 1), 2.0) == 102).all()
    assert (R.clahe_rgb(img, (1, 1), None) == 255).all()


def test_transposing_takes_swapped_tiles(rng):
    img = scene_u8(rng, 37, 53)
    t = np.ascontiguousarray(np.transpose(img, (1, 0, 2)))
    for tiles in ((2, 3), (3, 4)):
        out = R.clahe_rgb(img, tiles, 2.0)
        swapped = R.clahe_rgb(t, tiles[::-1], 2.0)
        assert np.array_equal(np.transpose(swapped, (1, 0, 2)), out)
    same = R.clahe_rgb(t, (2, 3), 2.0)                               # the unswapped grid is another operator
    assert not np.array_equal(np.transpose(same, (1, 0, 2)), R.clahe_rgb(img, (2, 3), 2.0))


def test_the_cases_of_the_gpu_tests_are_not_vacuous(rng):
    """On the 70 x 260 scene the operator moves most pixels, truncation differs from floor, and 0.3 .. 4.3 % of the channel
    values saturate as the contract records."""
    img = scene_u8(rng, 70, 260)
    base = R.clahe_rgb(img, (2, 3), 2.0)
    frac = lambda x: float((x != base).any(axis=2).mean())                              # noqa: E731
    assert frac(img) > 0.8
    half = R.clahe_rgb(img, (2, 3), 2.0, 0.5)
    assert float((R.clahe_rgb(img, (2, 3), 2.0, 0.5, truncate=True) != half).any(axis=2).mean()) > 0.02
    assert frac(R.clahe_rgb(img, (2, 3), None)) > 0.5 and frac(R.clahe_rgb(img, (2, 3), 4.0)) > 0.5
    wide = img.astype(np.int32) + R.delta(luma(img), (2, 3), 2.0)[..., None]
    assert 0.003 <= float(((wide < 0) | (wide > 255)).mean()) <= 0.043


# ---- settings --------------------------------------------------------------------------------------------------------------
def test_local_contrast_settings():
    s = LocalContrast()
    assert (s.tiles, s.clip_limit, s.strength) == ((8, 8), 2.0, 1.0) and (s.clip_q8, s.strength_q6) == (512, 64)
    assert LocalContrast(clip_limit=None).clip_q8 == 0 and LocalContrast(clip_limit=1).clip_q8 == 256
    assert LocalContrast(clip_limit=64.0).clip_q8 == 16384 and LocalContrast(strength=0).strength_q6 == 0
    assert LocalContrast(strength=0.0078125).strength_q6 == 1 and LocalContrast(strength=0.0078).strength_q6 == 0
    assert [LocalContrast(clip_limit=c).clip_q8 for c in (1.3, 2.7)] == [R.clip_q8(c) for c in (1.3, 2.7)]
    assert [LocalContrast(strength=c).strength_q6 for c in (0.3, 0.77)] == [R.strength_q6(c) for c in (0.3, 0.77)]
    assert LocalContrast([1, 16]).tiles == (1, 16) and LocalContrast((np.int64(3), 4)).tiles == (3, 4)
    assert check_local_contrast(None) is None and check_local_contrast(s) is s
    a = LocalContrast((3, 4), 4.0, 0.5)._arg()
    assert (a.tiles_y, a.tiles_x, a.clip_q8, a.strength_q6) == (3, 4, 1024, 32)
    for bad in ({"tiles": (0, 8)}, {"tiles": (8, 17)}, {"tiles": (8,)}, {"tiles": 8}, {"tiles": (8, 8, 8)},
                {"tiles": (8.0, 8)}, {"tiles": (True, 8)}, {"tiles": None}, {"tiles": "88"},
                {"clip_limit": 0.99}, {"clip_limit": 64.01}, {"clip_limit": math.inf}, {"clip_limit": math.nan},
                {"clip_limit": True}, {"clip_limit": "2"}, {"clip_limit": 0},
                {"strength": -0.01}, {"strength": 1.01}, {"strength": math.nan}, {"strength": False}, {"strength": None},
                {"strength": "1"}):
        with pytest.raises(ValueError):
            LocalContrast(**bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.strength = 0.5
    for bad in (True, 1, 2.0, (8, 8), "on"):
        with pytest.raises(ValueError):
            check_local_contrast(bad)
    with pytest.raises(ValueError):
        camera_isp.Camera16(camera_isp.bayer.BayerPattern.RGGB, local_contrast=1.0)


def test_shape_limits():
    lc = LocalContrast((3, 4))
    lcm.check_shape(3, 4, lc)
    lcm.check_shape(32768, 32768, lc)
    lcm.check_shape(0, 4, lc)                                        # (empty images pass: a no-op)
    lcm.check_shape(2, 0, lc)
    for H, W in ((2, 4), (3, 3), (32769, 8), (8, 32769)):
        with pytest.raises(ValueError):
            lcm.check_shape(H, W, lc)


def test_package_exports_local_contrast():
    import taichi_image_amd as ti
    assert ti.LocalContrast is LocalContrast and ti.local_contrast.clahe and ti.local_contrast.clahe_yuv420
    assert ti.local_contrast.apply and ti.local_contrast.check_local_contrast


def test_local_contrast_entry_points_validate_on_the_host():
    """Every bad setting, count, shape and pointer is refused before anything is launched (no device)."""
    from taichi_image_amd import _native
    names = {"mi_isp_local_contrast_workspace_bytes", "mi_isp_local_contrast_rgb_batch", "mi_isp_local_contrast_yuv420_batch"}
    assert names <= set(_native.SIGNATURES)
    L = _native.lib()
    assert L.mi_isp_version() == 1900
    good = _native.LocalContrast(8, 8, 512, 64)
    src = (ctypes.c_void_p * 2)(0x1000, 0x3000)
    dst = (ctypes.c_void_p * 2)(0x2000, 0x4000)
    ws = ctypes.c_void_p(0x10000)

    def refused(rc):
        assert rc == 1                                           # (1: a host check; 2 would be a launch error)
        assert b"local_contrast" in L.mi_isp_last_error()

    bad_settings = [_native.LocalContrast(0, 8, 512, 64), _native.LocalContrast(8, 17, 512, 64),
                    _native.LocalContrast(-1, 8, 512, 64), _native.LocalContrast(8, 8, 255, 64),
                    _native.LocalContrast(8, 8, 16385, 64), _native.LocalContrast(8, 8, -1, 64),
                    _native.LocalContrast(8, 8, 512, -1), _native.LocalContrast(8, 8, 512, 65)]
    for fn in (L.mi_isp_local_contrast_rgb_batch, L.mi_isp_local_contrast_yuv420_batch):
        for s in bad_settings:
            refused(fn(src, dst, 2, 16, 16, s, ws, None))
        refused(fn(src, dst, 2, 16, 16, None, ws, None))
        refused(fn(src, dst, -1, 16, 16, good, ws, None))
        refused(fn(src, dst, 2, -2, 16, good, ws, None))
        refused(fn(src, dst, 2, 16, -2, good, ws, None))
        refused(fn(src, dst, 2, 6, 16, good, ws, None))          # H < Ty
        refused(fn(src, dst, 2, 16, 6, good, ws, None))          # W < Tx
        refused(fn(src, dst, 2, 32770, 16, good, ws, None))
        refused(fn(src, dst, 2, 16, 32770, good, ws, None))
        refused(fn(None, dst, 2, 16, 16, good, ws, None))
        refused(fn(src, None, 2, 16, 16, good, ws, None))
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, None), 2, 16, 16, good, ws, None))
        refused(fn(src, dst, 2, 16, 16, good, None, None))       # no workspace
        refused(fn(src, dst, 2, 16, 16, good, ctypes.c_void_p(0x10004), None))
        assert fn(src, dst, 0, 16, 16, good, ws, None) == 0      # n == 0: a successful no-op
        assert fn(src, dst, 2, 0, 16, good, ws, None) == 0       # H * W == 0 too
        assert fn(src, dst, 2, 16, 0, good, ws, None) == 0
        assert fn(None, None, 0, 16, 16, good, None, None) == 0
    refused(L.mi_isp_local_contrast_yuv420_batch(src, dst, 2, 15, 16, good, ws, None))    # odd Y plane sides
    refused(L.mi_isp_local_contrast_yuv420_batch(src, dst, 2, 16, 15, good, ws, None))
    # the workspace: 256 u32 counters and 256 LUT bytes per tile and image
    assert L.mi_isp_local_contrast_workspace_bytes(3, good) == 3 * 64 * 1280
    assert L.mi_isp_local_contrast_workspace_bytes(33, _native.LocalContrast(16, 16, 0, 0)) == 33 * 256 * 1280
    assert L.mi_isp_local_contrast_workspace_bytes(0, good) == 0
    assert L.mi_isp_local_contrast_workspace_bytes(1, bad_settings[0]) == 0
    assert L.mi_isp_local_contrast_workspace_bytes(1, None) == 0


def test_scan_cli_takes_the_settings():
    from taichi_image_amd.scripts import tonemap_scan
    a = tonemap_scan.build_parser().parse_args(["--images", "x", "--local-contrast", "0.5", "--local-contrast-tiles", "4", "6",
                                                "--local-contrast-clip", "3"])
    assert (a.local_contrast, a.local_contrast_tiles, a.local_contrast_clip) == (0.5, [4, 6], 3.0)
    d = tonemap_scan.build_parser().parse_args(["--images", "x"])
    assert (d.local_contrast, d.local_contrast_tiles, d.local_contrast_clip) == (None, None, None)
    for bad in (["--local-contrast", "1.5"], ["--local-contrast", "-1"],
                ["--local-contrast", "1", "--local-contrast-tiles", "0", "8"],
                ["--local-contrast", "1", "--local-contrast-tiles", "8", "17"],
                ["--local-contrast", "1", "--local-contrast-clip", "0.5"],
                ["--local-contrast", "1", "--local-contrast-clip", "65"],
                ["--local-contrast-tiles", "4", "4"], ["--local-contrast-clip", "2"]):     # (settings without the flag)
        with pytest.raises(ValueError):                          # refused before any frame is read
            tonemap_scan.main(["--images", "/nonexistent"] + bad)
