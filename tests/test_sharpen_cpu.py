"""Output sharpening without a GPU: the NumPy statement of the contract (tests/sharpen_ref.py) pinned by hand, the
settings' checks in Python and in the C entry points, and the scan CLI's argument checks."""
import ctypes
import math

import numpy as np
import pytest

from oracle import isp_oracle as O
from taichi_image_amd import camera_isp
from taichi_image_amd.sharpen import Sharpen, check_sharpen
from tests import sharpen_ref as S

SETTINGS = [(1.5, 0, None), (1.5, 4, None), (1.5, 0, 0), (1.5, 0, 8), (8.0, 0, None), (0.0, 0, None)]
TRANSFORMS = ["none", "rotate_90", "rotate_180", "rotate_270", "transpose", "flip_horiz", "flip_vert", "transverse"]


def grey(row):
    """An (8, len(row), 3) grey image whose every row is `row` (R = G = B = v has luma v: 77 + 150 + 29 = 256)."""
    a = np.asarray(row, np.uint8)
    return np.repeat(np.tile(a[None, :, None], (8, 1, 1)), 3, axis=2)


def step(a, b, n=4):
    return grey([a] * n + [b] * n)


# ---- the restatement, pinned by hand ---------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("amount,threshold,overshoot", SETTINGS + [(8.0, 255, 0), (3.0, 7, 255)])
def test_flat_image_is_unchanged(radius, amount, threshold, overshoot):
    for v in (0, 1, 127, 255):
        img = np.full((9, 11, 3), v, np.uint8)
        assert np.array_equal(S.sharpen_rgb(img, amount, radius, threshold, overshoot), img)
    img = np.empty((6, 7, 3), np.uint8)
    img[...] = (200, 30, 90)                                       # flat colour
    assert np.array_equal(S.sharpen_rgb(img, amount, radius, threshold, overshoot), img)


@pytest.mark.parametrize("radius", [1, 2])
def test_amount_zero_is_the_identity(rng, radius):
    img = rng.integers(0, 256, (13, 17, 3)).astype(np.uint8)
    assert np.array_equal(S.sharpen_rgb(img, 0.0, radius), img)
    assert np.array_equal(S.sharpen_rgb(img, 0.0, radius, 3, 2), img)
    yuv = rng.integers(0, 256, (12, 10)).astype(np.uint8)
    assert np.array_equal(S.sharpen_yuv420(yuv, 0.0, radius), yuv)


@pytest.mark.parametrize("radius", [1, 2])
def test_one_pixel_and_one_row(rng, radius):
    one = np.array([[[10, 200, 30]]], np.uint8)
    assert np.array_equal(S.sharpen_rgb(one, 8.0, radius), one)    # every tap clamps onto the pixel
    row = grey([100] * 4 + [110] * 4)[:1]                          # (1, 8, 3): rows clamp, the step is as in a tall image
    want = {1: [100, 100, 100, 96, 114, 110, 110, 110], 2: [100, 100, 99, 95, 115, 111, 110, 110]}[radius]
    assert S.sharpen_rgb(row, 1.5, radius)[0, :, 0].tolist() == want
    col = np.transpose(row, (1, 0, 2))                             # (8, 1, 3)
    assert S.sharpen_rgb(col, 1.5, radius)[:, 0, 0].tolist() == want
    assert S.sharpen_rgb(np.zeros((0, 5, 3), np.uint8), 1.5, radius).shape == (0, 5, 3)


def test_step_edge_by_hand():
    """A vertical step 100 | 110 in a grey image (luma = the value).  The rows are equal, so the vertical pass multiplies
    the horizontal one by sum b.
    Radius 1 (S = 16, k = 10): d = 4 (2 L[x] - L[x-1] - L[x+1]) = -40 at the last 100, +40 at the first 110.
      amount 1.5 (A = 96): (-3840 + 512) >> 10 = floor(-3.25) = -4 (truncation gives -3); (3840 + 512) >> 10 = 4.
    Radius 2 (S = 256, k = 14): d = 16 (16 L[x] - sum b_j L[x+j-2]) = -160, -800, +800, +160 around the step.
      A = 96: (-15360 + 8192) >> 14 = floor(-0.4375) = -1 (truncation: 0); (-76800 + 8192) >> 14 = floor(-4.19) = -5
      (truncation: -4); (76800 + 8192) >> 14 = 5; (15360 + 8192) >> 14 = 1."""
    img = step(100, 110)
    r1 = S.sharpen_rgb(img, 1.5, 1)
    r2 = S.sharpen_rgb(img, 1.5, 2)
    for out, want in ((r1, [100, 100, 100, 96, 114, 110, 110, 110]), (r2, [100, 100, 99, 95, 115, 111, 110, 110])):
        for y in range(img.shape[0]):
            for ch in range(3):
                assert out[y, :, ch].tolist() == want
    # truncation toward zero is another filter, and only on the negative side
    assert S.sharpen_rgb(img, 1.5, 1, truncate=True)[0, :, 0].tolist() == [100, 100, 100, 97, 114, 110, 110, 110]
    assert S.sharpen_rgb(img, 1.5, 2, truncate=True)[0, :, 0].tolist() == [100, 100, 100, 96, 115, 111, 110, 110]
    # coring, radius 1: threshold 2 takes 2 S = 32 off |d| = 40: d' = -8, +8; (-768 + 512) >> 10 = -1, (768 + 512) >> 10 = 1
    assert S.sharpen_rgb(img, 1.5, 1, threshold=2)[0, :, 0].tolist() == [100, 100, 100, 99, 111, 110, 110, 110]
    # threshold 3: 48 >= 40, d' = 0, delta = 512 >> 10 = 0
    assert np.array_equal(S.sharpen_rgb(img, 1.5, 1, threshold=3), img)
    # the halo clamp, radius 1, amount 8 (A = 512): (-20480 + 512) >> 10 = floor(-19.5) = -20, (20480 + 512) >> 10 = 20,
    # so 80 | 130 without it; overshoot 5 clamps to [min3x3 - 5, max3x3 + 5] = [95, 115]; overshoot 0 to [100, 110]
    assert S.sharpen_rgb(img, 8.0, 1)[0, :, 0].tolist() == [100, 100, 100, 80, 130, 110, 110, 110]
    assert S.sharpen_rgb(img, 8.0, 1, overshoot=5)[0, :, 0].tolist() == [100, 100, 100, 95, 115, 110, 110, 110]
    assert np.array_equal(S.sharpen_rgb(img, 8.0, 1, overshoot=0), img)
    # the Y-plane form gives the same numbers on the plane and keeps the chroma rows
    yuv = np.concatenate([img[:, :, 0], np.full((4, 8), 77, np.uint8)])
    got = S.sharpen_yuv420(yuv, 1.5, 2)
    assert got[3].tolist() == [100, 100, 99, 95, 115, 111, 110, 110] and np.array_equal(got[8:], yuv[8:])


def test_saturation_at_0_and_255():
    """2 | 252, radius 1, amount 8: d = -+1000, delta = (-512000 + 512) >> 10 = -500 and +500: the bytes saturate."""
    out = S.sharpen_rgb(step(2, 252), 8.0, 1)
    assert out[0, :, 0].tolist() == [2, 2, 2, 0, 255, 252, 252, 252]
    # a coloured pixel saturates per channel: the same delta on R, G and B, each clamped on its own
    img = step(100, 110)
    img[:, :, 0] = np.where(img[:, :, 0] == 100, 2, 253)           # R far from G = B: luma 71 | 153, d = -+328
    dl = S.delta(S.luma(img), 8.0, 1)
    assert S.luma(img)[0].tolist() == [71] * 4 + [153] * 4 and dl[0].tolist() == [0, 0, 0, -164, 164, 0, 0, 0]
    out = S.sharpen_rgb(img, 8.0, 1)
    assert out[0, 3].tolist() == [0, 0, 0] and out[0, 4].tolist() == [255, 255, 255]
    out = S.sharpen_rgb(img, 1.0, 1)                               # delta -20 | +21: R saturates, G and B do not
    assert out[0, 3].tolist() == [0, 80, 80] and out[0, 4].tolist() == [255, 131, 131]


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", TRANSFORMS)
def test_sharpening_commutes_with_the_transforms(rng, radius, name):
    shapes = [(17, 17)] if name == "transverse" else [(17, 17), (9, 14), (1, 6)]
    for H, W in shapes:
        img = S.scene_u8(rng, H, W)
        for amount, threshold, overshoot in ((1.5, 0, None), (2.0, 1, 3)):
            a = O.transform(S.sharpen_rgb(img, amount, radius, threshold, overshoot), name)
            b = S.sharpen_rgb(np.ascontiguousarray(O.transform(img, name)), amount, radius, threshold, overshoot)
            assert np.array_equal(a, b), (name, H, W)


def test_the_cases_of_the_gpu_tests_are_not_vacuous(rng):
    """On a 70 x 131 scene at amount 1.5 the filter moves most pixels, and every variant moves the baseline's output."""
    img = S.scene_u8(rng, 70, 131)
    for radius in (1, 2):
        base = S.sharpen_rgb(img, 1.5, radius)
        frac = lambda x: float((x != base).any(axis=2).mean())                          # noqa: E731
        assert frac(img) > 0.8
        assert frac(S.sharpen_rgb(img, 1.5, radius, truncate=True)) > 0.2
        assert frac(S.sharpen_rgb(img, 1.5, radius, threshold=4)) > 0.5
        assert frac(S.sharpen_rgb(img, 1.5, radius, overshoot=0)) > 0.2
        assert frac(S.sharpen_rgb(img, 1.5, radius, overshoot=8)) > 0.02
        assert frac(S.sharpen_rgb(img, 8.0, radius)) > 0.8


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_sharpen_settings():
    s = Sharpen()
    assert (s.amount, s.radius, s.threshold, s.overshoot) == (1.0, 1, 0, None) and s.amount_q6 == 64
    assert Sharpen(1.5).amount_q6 == 96 and Sharpen(8).amount_q6 == 512 and Sharpen(0.0).amount_q6 == 0
    assert Sharpen(0.0078125).amount_q6 == 1 and Sharpen(0.0078).amount_q6 == 0     # floor(amount * 64 + 0.5)
    assert [Sharpen(a).amount_q6 for a in (0.3, 1.0, 2.7)] == [S.amount_q6(a) for a in (0.3, 1.0, 2.7)]
    assert Sharpen(2.0, 2, 255, 255).overshoot == 255 and Sharpen(overshoot=0).overshoot == 0
    assert check_sharpen(None) is None and check_sharpen(s) is s
    a = Sharpen(1.5, 2, 4, 8)._arg()
    assert (a.amount_q6, a.radius, a.threshold, a.overshoot) == (96, 2, 4, 8) and Sharpen()._arg().overshoot == -1
    for bad in ({"amount": -0.1}, {"amount": 8.01}, {"amount": math.inf}, {"amount": math.nan}, {"amount": "1"},
                {"amount": True}, {"amount": None}, {"radius": 0}, {"radius": 3}, {"radius": 1.0}, {"radius": True},
                {"threshold": -1}, {"threshold": 256}, {"threshold": 1.0}, {"threshold": True}, {"threshold": None},
                {"overshoot": -1}, {"overshoot": 256}, {"overshoot": 2.0}, {"overshoot": False}):
        with pytest.raises(ValueError):
            Sharpen(**bad)
    with pytest.raises(dataclass_frozen_error()):
        s.amount = 2.0
    for bad in (True, 1, 1.5, (1.5, 1), "on"):
        with pytest.raises(ValueError):
            check_sharpen(bad)
    with pytest.raises(ValueError):
        camera_isp.Camera16(camera_isp.bayer.BayerPattern.RGGB, sharpen=1.5)


def dataclass_frozen_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_package_exports_sharpen():
    import taichi_image_amd as ti
    assert ti.Sharpen is Sharpen and ti.sharpen.unsharp_mask and ti.sharpen.unsharp_mask_yuv420


def test_sharpen_entry_points_validate_on_the_host():
    """Every bad setting, count, shape and pointer is refused before anything is launched (no device)."""
    from taichi_image_amd import _native
    assert {"mi_isp_sharpen_rgb_batch", "mi_isp_sharpen_yuv420_batch"} <= set(_native.SIGNATURES)
    L = _native.lib()
    assert L.mi_isp_version() >= 1800
    good = _native.Sharpen(96, 1, 0, -1)
    src = (ctypes.c_void_p * 2)(0x1000, 0x3000)
    dst = (ctypes.c_void_p * 2)(0x2000, 0x4000)

    def refused(rc):
        assert rc == 1                                           # (1: a host check; 2 would be a launch error)
        assert b"sharpen" in L.mi_isp_last_error()

    for fn in (L.mi_isp_sharpen_rgb_batch, L.mi_isp_sharpen_yuv420_batch):
        for s in (_native.Sharpen(96, 0, 0, -1), _native.Sharpen(96, 3, 0, -1), _native.Sharpen(-1, 1, 0, -1),
                  _native.Sharpen(513, 1, 0, -1), _native.Sharpen(96, 1, -1, -1), _native.Sharpen(96, 1, 256, -1),
                  _native.Sharpen(96, 1, 0, -2), _native.Sharpen(96, 1, 0, 256)):
            refused(fn(src, dst, 2, 8, 8, s, None))
        refused(fn(src, dst, 2, 8, 8, None, None))
        refused(fn(src, dst, 0, 8, 8, good, None))               # n < 1
        refused(fn(src, dst, -1, 8, 8, good, None))
        refused(fn(src, dst, 2, -2, 8, good, None))
        refused(fn(src, dst, 2, 8, -1, good, None))
        refused(fn(None, dst, 2, 8, 8, good, None))
        refused(fn(src, None, 2, 8, 8, good, None))
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, 0x3000), 2, 8, 8, good, None))     # image 1 in place
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, None), 2, 8, 8, good, None))
        assert fn(src, dst, 2, 0, 8, good, None) == 0            # H * W == 0: a successful no-op
        assert fn(src, dst, 2, 8, 0, good, None) == 0
    refused(L.mi_isp_sharpen_yuv420_batch(src, dst, 2, 7, 8, good, None))                 # odd Y plane height


def test_scan_cli_takes_the_settings():
    from taichi_image_amd.scripts import tonemap_scan
    a = tonemap_scan.build_parser().parse_args(["--images", "x", "--sharpen", "1.5", "--sharpen-radius", "2",
                                                "--sharpen-threshold", "4", "--sharpen-overshoot", "8"])
    assert (a.sharpen, a.sharpen_radius, a.sharpen_threshold, a.sharpen_overshoot) == (1.5, 2, 4, 8)
    d = tonemap_scan.build_parser().parse_args(["--images", "x"])
    assert (d.sharpen, d.sharpen_radius, d.sharpen_threshold, d.sharpen_overshoot) == (None, 1, 0, None)
    for bad in (["--sharpen", "9"], ["--sharpen", "-1"], ["--sharpen", "1.5", "--sharpen-radius", "3"],
                ["--sharpen", "1.5", "--sharpen-threshold", "256"], ["--sharpen", "1.5", "--sharpen-overshoot", "-1"],
                ["--sharpen-radius", "2"]):                       # (the last: a setting without --sharpen)
        with pytest.raises(ValueError):                          # refused before any frame is read
            tonemap_scan.main(["--images", "/nonexistent"] + bad)
