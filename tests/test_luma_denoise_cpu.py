"""Luma noise reduction without a GPU: the NumPy statement of the contract (tests/luma_denoise_ref.py) pinned by hand and
by its properties, the noise it removes from a flat image, the settings' checks in Python and in the C entry points, the
scan CLI's argument checks, the kernel's division helper against integer division (a host program), and the inputs of
tests/test_gpu_luma_denoise.py shown to tell the contract from its mutants."""
import ctypes
import dataclasses
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import isp_oracle as O
from taichi_image_amd import camera_isp
from taichi_image_amd.luma_denoise import LumaDenoise, check_luma_denoise
from tests import chroma_denoise_ref as C
from tests import luma_denoise_ref as Y
from tests import sharpen_ref as S

SETTINGS = [(6, 14, 1.0), (255, 255, 1.0), (6, 14, 0.5), (2, 14, 1.0), (6, 3, 1.0), (6, 14, 0.0)]          # (t0, t1, strength)
TRANSFORMS = ["none", "rotate_90", "rotate_180", "rotate_270", "transpose", "flip_horiz", "flip_vert", "transverse"]
RADII = [1, 2, 3]
GPU_SHAPES_FROM_30_ROWS = [(31, 33), (64, 64), (134, 264), (131, 261), (35, 132)]     # of tests/test_gpu_luma_denoise.py
GPU_YUV_SHAPES_FROM_30_ROWS = [(30, 34), (64, 64), (134, 264), (36, 132), (130, 262)]


def grey(rows):
    """The (H, W, 3) u8 image with R = G = B = rows (its luma is rows: 77 + 150 + 29 = 256)."""
    a = np.asarray(rows, np.uint8)
    return np.repeat(a[..., None], 3, axis=2)


# ---- the restatement, pinned by hand ---------------------------------------------------------------------------------
def test_one_pixel_is_the_identity(rng):
    """A 1 x 1 image has one tap, the pixel: n = 1, s = L, m = (2 L + 1) // 2 = L, delta = 32 >> 6 = 0."""
    for v in (0, 1, 100, 255):
        for r in RADII:
            for t0, t1, strength in SETTINGS:
                assert np.array_equal(Y.luma_denoise_rgb(grey([[v]]), r, t0, t1, strength), grey([[v]]))
    img = rng.integers(0, 256, (1, 1, 3)).astype(np.uint8)
    assert np.array_equal(Y.luma_denoise_rgb(img, 3, 255, 255, 1.0), img)


def test_a_row_of_three_by_hand():
    """L = 10 13 11, radius 1 (the rows above and below are outside the image: no taps), t0 = t1 = 3, strength 1 (S = 64):
      p0 (10): taps 10, 13 (|3| <= 3: the boundary counts)  n = 2, s = 23, m = (46 + 2) // 4 = 12 (11.5: the tie goes up)
               d = 2, delta = (128 + 32) >> 6 = 2                                                         -> 12
      p1 (13): taps 10, 13, 11                              n = 3, s = 34, m = (68 + 3) // 6 = 11 (11.33)
               d = -2, delta = (-128 + 32) >> 6 = -2  (truncation: d = -7 / 6 -> -1, delta = -32 / 64 -> 0) -> 11
      p2 (11): taps 13, 11                                  n = 2, s = 24, m = (48 + 2) // 4 = 12         -> 12"""
    img = grey([[10, 13, 11]])
    n, s = Y.window(S.luma(img), 1, 3)
    assert n.tolist() == [[2, 3, 2]] and s.tolist() == [[23, 34, 24]]
    assert Y.delta(S.luma(img), 1, 3, 3, 1.0).tolist() == [[2, -2, 1]]
    assert np.array_equal(Y.luma_denoise_rgb(img, 1, 3, 3, 1.0), grey([[12, 11, 12]]))
    assert np.array_equal(Y.luma_denoise_rgb(grey([[10], [13], [11]]), 1, 3, None, 1.0), grey([[12], [11], [12]]))   # as a column
    # radius 2 and 3 reach across the row: p0 and p2 see each other, every pixel has n = 3, s = 34, m = 11
    assert np.array_equal(Y.luma_denoise_rgb(img, 3, 3, 3, 1.0), grey([[11, 11, 11]]))
    # truncation toward zero is another filter, and only on the negative side
    assert Y.delta(S.luma(img), 1, 3, 3, 1.0, truncate=True).tolist() == [[2, 0, 1]]
    # strength 0.5 (S = 32): (64 + 32) >> 6 = 1, (-64 + 32) >> 6 = -1 (truncation: 0), (32 + 32) >> 6 = 1
    assert Y.delta(S.luma(img), 1, 3, 3, 0.5).tolist() == [[1, -1, 1]]
    # t = 2 drops the pair 10, 13: p0 alone; p1 with 11: s = 24, m = 12, d = -1; p2 as before
    assert np.array_equal(Y.luma_denoise_rgb(img, 1, 2, 2, 1.0), grey([[10, 12, 12]]))
    # clamped border taps would count p0 six times and 13 three times: n = 9, s = 99, m = 207 // 18 = 11 (NOT the contract)
    nc, sc = Y.window(S.luma(img), 1, 3, clamp_border=True)
    assert (nc[0, 0], sc[0, 0]) == (9, 99)
    assert Y.delta(S.luma(img), 1, 3, 3, 1.0, clamp_border=True)[0, 0] == 1
    # a coloured pixel takes the delta on every channel, up to the clip
    col = np.array([[[250, 0, 40], [255, 2, 30], [251, 1, 36]]], np.uint8)
    dl = Y.delta(S.luma(col), 1, 255, 255, 1.0)              # L = 80 81 80: n = 2, 3, 2; m = 81, 80, 81
    assert dl.tolist() == [[1, -1, 1]]
    assert np.array_equal(Y.luma_denoise_rgb(col, 1, 255, 255, 1.0), np.clip(col.astype(int) + dl[..., None], 0, 255))


def test_the_threshold_moves_with_the_luma():
    """T = t0 + (((t1 - t0) L + 128) >> 8), the shift a floor: from t0 at L = 0 to within one code of t1 at L = 255."""
    L = np.array([[0, 10, 128, 255]])
    assert Y.thresholds(L, 0, 255).tolist() == [[0, 10, 128, 254]]          # (2550 + 128) >> 8 = 10, (65025 + 128) >> 8 = 254
    assert Y.thresholds(L, 255, 0).tolist() == [[255, 245, 128, 1]]         # (-65025 + 128) >> 8 = -254 (floor of -253.5)
    assert Y.thresholds(L, 6, 14).tolist() == [[6, 6, 10, 14]]
    assert Y.thresholds(L, 6, 3).tolist() == [[6, 6, 5, 3]]
    assert Y.thresholds(L, 6, None).tolist() == [[6, 6, 6, 6]] == Y.thresholds(L, 6, 14, fixed_threshold=True).tolist()
    allL = np.arange(256)[None]
    for t0 in (0, 1, 6, 200, 255):
        for t1 in (0, 3, 14, 255):
            T = Y.thresholds(allL, t0, t1)
            assert T.min() >= 0 and T.max() <= 255 and T[0, 0] == t0 and abs(int(T[0, 255]) - t1) <= 1
    # a dark pair 4 apart stays (T(10) = 2, T(14) = 2 + (296 >> 8) = 3), a bright pair 4 apart meets: T(240) = 2 + (3008 >> 8)
    # = 13, n = 2, s = 484, m = (968 + 2) // 4 = 242 for both pixels; with threshold_bright ignored it stays too
    dark, bright = grey([[10, 14]]), grey([[240, 244]])
    assert np.array_equal(Y.luma_denoise_rgb(dark, 1, 2, 14, 1.0), dark)
    assert np.array_equal(Y.luma_denoise_rgb(bright, 1, 2, 14, 1.0), grey([[242, 242]]))
    assert np.array_equal(Y.luma_denoise_rgb(bright, 1, 2, 14, 1.0, fixed_threshold=True), bright)


def test_threshold_255_gives_the_mean_of_the_taps_inside_the_image(rng):
    for H, W in ((1, 9), (9, 1), (5, 5), (13, 17)):
        L = rng.integers(0, 256, (H, W))
        for r in RADII:
            want = np.empty((H, W), np.int64)
            for y in range(H):
                for x in range(W):
                    w = L[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1]
                    want[y, x] = math.floor(w.sum() / w.size + 0.5)
            n, s = Y.window(L, r, 255)
            assert np.array_equal((2 * s + n) // (2 * n), want)
            assert np.array_equal(Y.delta(L, r, 255, 255, 1.0), want - L)
            assert np.array_equal(Y.luma_denoise_rgb(grey(L), r, 255, None, 1.0), grey(want))


# ---- the properties the contract lists -----------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
def test_a_step_edge_is_kept(rng, radius):
    """Two noisy flat halves 50 codes apart, thresholds below the step: no tap crosses the edge, and a tap across it counts as
    little as one outside the image, so the filter of the image is the filter of each half on its own."""
    left = np.clip(50 + np.rint(rng.normal(0, 2, (20, 11))), 0, 255).astype(np.uint8)
    right = np.clip(100 + np.rint(rng.normal(0, 2, (20, 12))), 0, 255).astype(np.uint8)
    img = grey(np.concatenate([left, right], axis=1))
    out = Y.luma_denoise_rgb(img, radius, 12, 12, 1.0)
    assert not np.array_equal(out, img)
    assert np.array_equal(out[:, :11], Y.luma_denoise_rgb(grey(left), radius, 12, 12, 1.0))
    assert np.array_equal(out[:, 11:], Y.luma_denoise_rgb(grey(right), radius, 12, 12, 1.0))
    clean = grey(np.concatenate([np.full((9, 7), 50), np.full((9, 6), 100)], axis=1))
    assert np.array_equal(Y.luma_denoise_rgb(clean, radius, 12, 30, 1.0), clean)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("t0,t1,strength", SETTINGS)
def test_flat_images_and_strength_zero_are_identities(rng, radius, t0, t1, strength):
    for colour in ((0, 0, 0), (255, 255, 255), (200, 30, 90), (1, 254, 7)):
        img = np.empty((7, 9, 3), np.uint8)
        img[...] = colour
        assert np.array_equal(Y.luma_denoise_rgb(img, radius, t0, t1, strength), img)
    img = rng.integers(0, 256, (13, 17, 3)).astype(np.uint8)
    assert np.array_equal(Y.luma_denoise_rgb(img, radius, t0, t1, 0.0), img)
    yuv = rng.integers(0, 256, (12, 10)).astype(np.uint8)
    assert np.array_equal(Y.luma_denoise_yuv420(yuv, radius, t0, t1, 0.0), yuv)


@pytest.mark.parametrize("radius", RADII)
def test_the_delta_is_within_the_threshold(rng, radius):
    for img in (S.scene_u8(rng, 40, 52), rng.integers(0, 256, (21, 33, 3)).astype(np.uint8)):
        L = S.luma(img)
        for t0, t1, strength in SETTINGS + [(0, 0, 1.0), (40, 0, 0.7)]:
            dl = Y.delta(L, radius, t0, t1, strength)
            assert (np.abs(dl) <= Y.thresholds(L, t0, t1)).all()
    assert np.array_equal(Y.luma_denoise_rgb(img, radius, 0, 0, 1.0), img)      # T = 0: only equal lumas count, m = L


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", TRANSFORMS)
def test_the_operator_commutes_with_the_transforms_at_odd_sizes(rng, radius, name):
    # (the transverse transform is defined for square images only)
    for H, W in ((1, 1), (7, 7), (9, 9)) if name == "transverse" else ((1, 1), (1, 7), (5, 1), (7, 11), (9, 9), (15, 6)):
        img = S.scene_u8(rng, H, W, sigma=0.04)
        for t0, t1, strength in ((6, 14, 1.0), (255, 255, 0.5)):
            a = O.transform(Y.luma_denoise_rgb(img, radius, t0, t1, strength), name)
            b = Y.luma_denoise_rgb(np.ascontiguousarray(O.transform(img, name)), radius, t0, t1, strength)
            assert np.array_equal(a, b), (name, H, W)


def test_the_planar_form_filters_the_y_plane_alone(rng):
    yuv = rng.integers(0, 256, (18, 10)).astype(np.uint8)
    yuv[:12] = np.clip(120 + np.rint(rng.normal(0, 3, (12, 10))), 0, 255).astype(np.uint8)
    out = Y.luma_denoise_yuv420(yuv, 2, 12, None, 1.0)
    assert np.array_equal(out[12:], yuv[12:]) and not np.array_equal(out[:12], yuv[:12])
    assert np.array_equal(out[:12], Y.luma_denoise_rgb(grey(yuv[:12]), 2, 12, None, 1.0)[..., 0])
    assert Y.luma_denoise_yuv420(np.zeros((0, 8), np.uint8)).shape == (0, 8)


@pytest.mark.parametrize("radius,bound", [(1, 0.2), (2, 0.1), (3, 0.05)])
def test_residual_noise_on_a_flat_image(radius, bound):
    """Code 100 plus Gaussian noise of sigma 2 on 256 x 256 pixels, thresholds 12 / 12 (6 sigma: nearly every tap counts),
    strength 1: the luma variance that is left, as a fraction of the input's.  The ideal box mean leaves 1 / 9, 1 / 25 and
    1 / 49; the integer mean adds its rounding (a variance of about 1 / 12 code^2, 0.02 of the input's 4)."""
    rng = np.random.default_rng(20)
    L = np.clip(100 + np.rint(rng.normal(0, 2, (256, 256))), 0, 255).astype(np.uint8)
    out = Y.luma_denoise_rgb(grey(L), radius, 12, 12, 1.0)
    ratio = S.luma(out).var() / L.astype(np.float64).var()
    print(f"radius {radius}: residual variance ratio {ratio:.4f} (bound {bound})")
    assert ratio < bound


def check_not_vacuous(ref_fn, img, radius, what):
    """The references of the SETTINGS in order: each differs from its input (strength 0 excepted, the identity), from the
    setting before it, and from the three mutants of the restatement (clamped border taps that count, truncation toward
    zero, threshold_bright ignored - compared only where t0 != t1)."""
    refs = [ref_fn(img, radius, t0, t1, strength) for t0, t1, strength in SETTINGS]
    for k, ref in enumerate(refs):
        t0, t1, strength = SETTINGS[k]
        if k > 0:
            assert not np.array_equal(ref, refs[k - 1]), f"{what}: settings {k - 1} and {k} give the same output"
        if strength > 0:
            assert not np.array_equal(ref, img), f"{what}: setting {k} leaves the input as it is"
            assert not np.array_equal(ref, ref_fn(img, radius, t0, t1, strength, clamp_border=True)), \
                f"{what}: setting {k} does not see clamped border taps"
            assert not np.array_equal(ref, ref_fn(img, radius, t0, t1, strength, truncate=True)), \
                f"{what}: setting {k} does not see truncation toward zero"
            if t0 != t1:
                assert not np.array_equal(ref, ref_fn(img, radius, t0, t1, strength, fixed_threshold=True)), \
                    f"{what}: setting {k} does not see a fixed threshold"
        else:
            assert np.array_equal(ref, img)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", GPU_SHAPES_FROM_30_ROWS)
def test_the_inputs_of_the_gpu_tests_are_not_vacuous(radius, H, W):
    """What tests/test_gpu_luma_denoise.py relies on: on the scene it uses (the same seed), at every shape of at least 30
    rows, every setting's reference differs from its input, from its neighbour and from each mutant."""
    check_not_vacuous(Y.luma_denoise_rgb, S.scene_u8(np.random.default_rng(H * 1000 + W), H, W), radius,
                      f"scene {H}x{W} R={radius}")


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", GPU_YUV_SHAPES_FROM_30_ROWS)
def test_the_planar_inputs_of_the_gpu_tests_are_not_vacuous(radius, H, W):
    check_not_vacuous(Y.luma_denoise_yuv420, C.scene_yuv420(np.random.default_rng(H * 1000 + W), H, W), radius,
                      f"planar scene {H}x{W} R={radius}")


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_luma_denoise_settings():
    s = LumaDenoise()
    assert (s.radius, s.threshold, s.threshold_bright, s.strength) == (2, 6, None, 1.0) and s.strength_q6 == 64
    assert LumaDenoise(strength=0.5).strength_q6 == 32 and LumaDenoise(strength=0).strength_q6 == 0
    assert LumaDenoise(strength=0.0078125).strength_q6 == 1 and LumaDenoise(strength=0.0078).strength_q6 == 0
    assert [LumaDenoise(strength=a).strength_q6 for a in (0.3, 0.7, 1.0)] == [Y.strength_q6(a) for a in (0.3, 0.7, 1.0)]
    assert LumaDenoise(3, 255, 255, 1).radius == 3 and LumaDenoise(1, 0, 0, 0.25).threshold == 0
    assert check_luma_denoise(None) is None and check_luma_denoise(s) is s
    a = LumaDenoise(3, 5, 7, 0.5)._arg()
    assert (a.radius, a.threshold, a.threshold_bright, a.strength_q6) == (3, 5, 7, 32)
    a = LumaDenoise(1, 9)._arg()                                  # None: the same as threshold
    assert (a.radius, a.threshold, a.threshold_bright, a.strength_q6) == (1, 9, 9, 64)
    for bad in ({"radius": 0}, {"radius": 4}, {"radius": 1.0}, {"radius": True}, {"radius": None},
                {"threshold": -1}, {"threshold": 256}, {"threshold": 6.0}, {"threshold": True}, {"threshold": None},
                {"threshold_bright": -1}, {"threshold_bright": 256}, {"threshold_bright": 12.0}, {"threshold_bright": False},
                {"strength": -0.1}, {"strength": 1.01}, {"strength": math.inf}, {"strength": math.nan}, {"strength": "1"},
                {"strength": True}, {"strength": None}):
        with pytest.raises(ValueError):
            LumaDenoise(**bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.strength = 0.5
    for bad in (True, 1, 0.5, (2, 6, None), "on"):
        with pytest.raises(ValueError):
            check_luma_denoise(bad)
    with pytest.raises(ValueError):
        camera_isp.Camera16(camera_isp.bayer.BayerPattern.RGGB, luma_denoise=1.0)


def test_package_exports_luma_denoise():
    import taichi_image_amd as ti
    assert ti.LumaDenoise is LumaDenoise
    assert ti.luma_denoise.luma_denoise and ti.luma_denoise.luma_denoise_yuv420 and ti.luma_denoise.apply
    assert ti.luma_denoise.check_luma_denoise is check_luma_denoise


def test_luma_denoise_entry_points_validate_on_the_host():
    """Every bad setting, count, shape, pointer and overlap is refused before anything is launched (no device)."""
    from taichi_image_amd import _native
    assert {"mi_isp_luma_denoise_rgb_batch", "mi_isp_luma_denoise_yuv420_batch"} <= set(_native.SIGNATURES)
    L = _native.lib()
    good = _native.LumaDenoise(2, 6, 14, 64)
    src = (ctypes.c_void_p * 2)(0x1000, 0x3000)
    dst = (ctypes.c_void_p * 2)(0x2000, 0x4000)

    def refused(rc):
        assert rc == 1                                           # (1: a host check; 2 would be a launch error)
        assert b"luma_denoise" in L.mi_isp_last_error()

    for fn, size in ((L.mi_isp_luma_denoise_rgb_batch, 8 * 8 * 3), (L.mi_isp_luma_denoise_yuv420_batch, 8 * 8 * 3 // 2)):
        for s in (_native.LumaDenoise(0, 6, 14, 64), _native.LumaDenoise(4, 6, 14, 64), _native.LumaDenoise(2, -1, 14, 64),
                  _native.LumaDenoise(2, 256, 14, 64), _native.LumaDenoise(2, 6, -1, 64), _native.LumaDenoise(2, 6, 256, 64),
                  _native.LumaDenoise(2, 6, 14, -1), _native.LumaDenoise(2, 6, 14, 65)):
            refused(fn(src, dst, 2, 8, 8, s, None))
        refused(fn(src, dst, 2, 8, 8, None, None))
        refused(fn(src, dst, -1, 8, 8, good, None))
        refused(fn(src, dst, 2, -2, 8, good, None))
        refused(fn(src, dst, 2, 8, -2, good, None))
        refused(fn(None, dst, 2, 8, 8, good, None))
        refused(fn(src, None, 2, 8, 8, good, None))
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, 0x3000), 2, 8, 8, good, None))     # image 1 in place
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, None), 2, 8, 8, good, None))
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, 0x3000 + size - 1), 2, 8, 8, good, None))      # output 1 into input 1
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, 0x3000 - size + 1), 2, 8, 8, good, None))
        refused(fn(src, (ctypes.c_void_p * 2)(0x1000 + size - 1, 0x4000), 2, 8, 8, good, None))      # output 0 into input 0
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, 0x2000 + size - 1), 2, 8, 8, good, None))      # the outputs overlap
        refused(fn(src, (ctypes.c_void_p * 2)(0x3000 + 1, 0x4000), 2, 8, 8, good, None))             # output 0 into input 1
        assert fn(src, (ctypes.c_void_p * 2)(0x1000 + size, 0x3000 + size), 0, 8, 8, good, None) == 0
        assert fn(src, dst, 0, 8, 8, good, None) == 0            # n == 0 and H * W == 0: successful no-ops
        assert fn(src, dst, 2, 0, 8, good, None) == 0
        assert fn(src, dst, 2, 8, 0, good, None) == 0
    refused(L.mi_isp_luma_denoise_yuv420_batch(src, dst, 2, 7, 8, good, None))            # odd Y plane sides
    refused(L.mi_isp_luma_denoise_yuv420_batch(src, dst, 2, 8, 7, good, None))


def test_scan_cli_takes_the_settings():
    from taichi_image_amd.scripts import tonemap_scan
    a = tonemap_scan.build_parser().parse_args(["--images", "x", "--luma-denoise", "0.5", "--luma-denoise-radius", "3",
                                                "--luma-denoise-thresholds", "4", "9"])
    assert (a.luma_denoise, a.luma_denoise_radius, a.luma_denoise_thresholds) == (0.5, 3, [4, 9])
    d = tonemap_scan.build_parser().parse_args(["--images", "x"])
    assert (d.luma_denoise, d.luma_denoise_radius, d.luma_denoise_thresholds) == (None, None, None)
    for bad in (["--luma-denoise", "1.5"], ["--luma-denoise", "-1"], ["--luma-denoise", "1", "--luma-denoise-radius", "4"],
                ["--luma-denoise", "1", "--luma-denoise-radius", "0"],
                ["--luma-denoise", "1", "--luma-denoise-thresholds", "256", "12"],
                ["--luma-denoise", "1", "--luma-denoise-thresholds", "6", "-1"],
                ["--luma-denoise-radius", "2"], ["--luma-denoise-thresholds", "6", "14"]):       # (the last two: no STRENGTH)
        with pytest.raises(ValueError):                          # refused before any frame is read
            tonemap_scan.main(["--images", "/nonexistent"] + bad)


# ---- the kernel's division ---------------------------------------------------------------------------------------------
def test_the_kernels_division_is_integer_division():
    """ydn::mean_ties_up_rcp, ydn::mean_ties_up and ydn::threshold_at of csrc/isp_luma_denoise.h, compiled for the host, against
    integer arithmetic over their whole domains (tests/check_luma_denoise_div.cpp)."""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "check")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", os.path.join(here, "check_luma_denoise_div.cpp"), "-o", exe],
                       check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok") == 51 and "mean ok" in out.stdout and "threshold ok" in out.stdout, out.stdout
