"""Chroma noise reduction without a GPU: the NumPy statement of the contract (tests/chroma_denoise_ref.py) pinned by hand
and by its properties, the settings' checks in Python and in the C entry points, the scan CLI's argument checks, and the
kernel's division helper against floor division (a host program)."""
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
from taichi_image_amd.chroma_denoise import ChromaDenoise, check_chroma_denoise
from tests import chroma_denoise_ref as C
from tests import sharpen_ref as S

SETTINGS = [(8, 12, 1.0), (255, 255, 1.0), (8, 12, 0.5), (2, 12, 1.0), (8, 3, 1.0), (8, 12, 0.0)]       # (tl, tc, strength)
TRANSFORMS = ["none", "rotate_90", "rotate_180", "rotate_270", "transpose", "flip_horiz", "flip_vert", "transverse"]
RADII = [1, 2, 3]


def cells_image(cells):
    """An image whose 2 x 2 cells are flat: cells is rows of (R, G, B)."""
    a = np.asarray(cells, np.uint8)
    return np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)


# ---- the restatement, pinned by hand ---------------------------------------------------------------------------------
def test_one_cell_is_the_identity(rng):
    """A 2 x 2 image is one cell: T = {p}, n = 1, DB = DR = 0, db = dr = 256 // 512 = 0, dg = 32768 >> 16 = 0.  The same
    holds for 1 x 1, 1 x 2 and 2 x 1, whose cell counts its pixels twice."""
    for shape in ((2, 2), (1, 1), (1, 2), (2, 1)):
        img = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
        for r in RADII:
            assert np.array_equal(C.chroma_denoise_rgb(img, r, 255, 255, 1.0), img)
    yuv = rng.integers(0, 256, (3, 2)).astype(np.uint8)
    assert np.array_equal(C.chroma_denoise_yuv420(yuv, 3, 255, 255, 1.0), yuv)


def test_four_cells_by_hand():
    """A 4 x 4 image of four flat cells, radius 1 (every cell is in every window), tl = 8 (4 tl = 32), tc = 12 (4 tc = 48),
    strength 1 (S = 64).  L = (77 R + 150 G + 29 B + 128) >> 8, a flat cell has SL = 4 L, SB = 4 (B - L), SR = 4 (R - L):
      A (0, 0) = (100, 100, 100): L = 25728 >> 8 = 100   SL 400  SB   0  SR   0
      B (0, 1) = (111,  96, 100): L = 25975 >> 8 = 101   SL 404  SB  -4  SR  40
      C (1, 0) = (100, 100, 120): L = 26308 >> 8 = 102   SL 408  SB  72  SR  -8
      D (1, 1) = (100, 104, 100): L = 26328 >> 8 = 102   SL 408  SB  -8  SR  -8
    (differences below as q - p: SL, SB, SR)
    A: B passes (4, -4, 40), C fails (SB 72 > 48), D passes (8, -8, -8): n = 3, DB = -12, DR = 32
       db = (-1536 + 768) // 1536 = -1 (truncation: 0), dr = (4096 + 768) // 1536 = 3,
       dg = ((-(231 - 29)) * 437 + 32768) >> 16 = -55506 >> 16 = -1                              -> (103,  99,  99)
    B: A passes (-4, 4, -40), C fails (SB 76), D passes (4, -4, -48: |SR| = 48 <= 48, the boundary): n = 3, DB = 0, DR = -88
       db = 768 // 1536 = 0, dr = (-11264 + 768) // 1536 = -7 (truncation: -6),
       dg = (539 * 437 + 32768) >> 16 = 268311 >> 16 = 4                                         -> (104, 100, 100)
    C: A, B, D fail (SB -72, -76, -80): n = 1, db = dr = 256 // 512 = 0, dg = 32768 >> 16 = 0     -> unchanged
    D: A passes (-8, 8, 8), B passes (-4, 4, 48), C fails (SB 80): n = 3, DB = 12, DR = 56
       db = (1536 + 768) // 1536 = 1, dr = (7168 + 768) // 1536 = 5,
       dg = ((-(385 + 29)) * 437 + 32768) >> 16 = -148150 >> 16 = -3                             -> (105, 101, 101)"""
    img = cells_image([[(100, 100, 100), (111, 96, 100)], [(100, 100, 120), (100, 104, 100)]])
    SL, SB, SR = C.cells_rgb(img)
    assert SL.tolist() == [[400, 404], [408, 408]] and SB.tolist() == [[0, -4], [72, -8]] and SR.tolist() == [[0, 40], [-8, -8]]
    n, DB, DR = C.window(SL, SB, SR, 1, 8, 12)
    assert n.tolist() == [[3, 3], [1, 3]] and DB.tolist() == [[-12, 0], [0, 12]] and DR.tolist() == [[32, -88], [0, 56]]
    db, dr, dg = C.deltas(SL, SB, SR, 1, 8, 12, 1.0)
    assert db.tolist() == [[-1, 0], [0, 1]] and dr.tolist() == [[3, -7], [0, 5]] and dg.tolist() == [[-1, 4], [0, -3]]
    want = cells_image([[(103, 99, 99), (104, 100, 100)], [(100, 100, 120), (105, 101, 101)]])
    assert np.array_equal(C.chroma_denoise_rgb(img, 1, 8, 12, 1.0), want)
    # the same cells at radius 2 and 3: the grid bounds the window
    assert np.array_equal(C.chroma_denoise_rgb(img, 3, 8, 12, 1.0), want)
    # truncation toward zero is another filter, and only on the negative side: A's db becomes 0, B's dr -6
    t = C.deltas(SL, SB, SR, 1, 8, 12, 1.0, truncate=True)
    assert t[0].tolist() == [[0, 0], [0, 1]] and t[1].tolist() == [[3, -6], [0, 5]]
    # a chroma threshold of 11 (44 < 48) drops D from B's window and B from D's
    n11, _, _ = C.window(SL, SB, SR, 1, 8, 11)
    assert n11.tolist() == [[3, 2], [1, 2]]
    # a luma threshold of 1 (4 < 8) drops D from A's window and A from D's; 4 <= 4 keeps the pairs A B and B D
    n1, _, _ = C.window(SL, SB, SR, 1, 1, 12)
    assert n1.tolist() == [[2, 3], [1, 2]]
    # clamped border taps would count A five times in its own 3 x 3 window, B and D once more each (NOT the contract)
    nc, _, _ = C.window(SL, SB, SR, 1, 8, 12, clamp_border=True)
    assert nc.tolist() == [[7, 8], [4, 7]]
    # strength 0.5 (S = 32): dr = (2048 + 768) // 1536 = 1, (-5632 + 768) // 1536 = -4, (3584 + 768) // 1536 = 2
    assert C.deltas(SL, SB, SR, 1, 8, 12, 0.5)[1].tolist() == [[1, -4], [0, 2]]


def test_four_chroma_samples_by_hand():
    """The planar form of a 4 x 4 image: SL = the four Y, SB = 4 U, SR = 4 V.  Y = 100 | 101 / 102 | 102 per cell, U =
    (128, 127 / 146, 126), V = (128, 138 / 126, 126): SL, SB - 512 = (0, -4 / 72, -8) and SR - 512 = (0, 40 / -8, -8) are
    the cells of test_four_cells_by_hand, so n, db and dr are the same: U' = U + db, V' = V + dr, Y as it is."""
    y = np.repeat(np.repeat(np.array([[100, 101], [102, 102]], np.uint8), 2, 0), 2, 1)
    yuv = np.concatenate([y.ravel(), np.array([128, 127, 146, 126, 128, 138, 126, 126], np.uint8)]).reshape(6, 4)
    out = C.chroma_denoise_yuv420(yuv, 1, 8, 12, 1.0)
    assert np.array_equal(out[:4], y)
    assert out[4].tolist() == [127, 127, 146, 127] and out[5].tolist() == [131, 131, 126, 131]


# ---- the properties the contract lists -----------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
def test_strength_zero_is_the_identity(rng, radius):
    img = rng.integers(0, 256, (13, 17, 3)).astype(np.uint8)
    assert np.array_equal(C.chroma_denoise_rgb(img, radius, 255, 255, 0.0), img)
    scene = S.scene_u8(rng, 20, 24)
    assert np.array_equal(C.chroma_denoise_rgb(scene, radius, 8, 12, 0.0), scene)
    yuv = rng.integers(0, 256, (12, 10)).astype(np.uint8)
    assert np.array_equal(C.chroma_denoise_yuv420(yuv, radius, 255, 255, 0.0), yuv)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("tl,tc,strength", SETTINGS)
def test_grey_and_flat_images_are_unchanged(rng, radius, tl, tc, strength):
    """R = G = B has L = R (77 + 150 + 29 = 256), so SB = SR = 0 everywhere and every delta is 0; a flat colour has every
    SB(q) - SB(p) = 0."""
    g = rng.integers(0, 256, (11, 14)).astype(np.uint8)
    grey = np.repeat(g[..., None], 3, axis=2)
    assert np.array_equal(C.chroma_denoise_rgb(grey, radius, tl, tc, strength), grey)
    for colour in ((0, 0, 0), (255, 255, 255), (200, 30, 90), (1, 254, 7)):
        img = np.empty((7, 9, 3), np.uint8)
        img[...] = colour
        assert np.array_equal(C.chroma_denoise_rgb(img, radius, tl, tc, strength), img)


@pytest.mark.parametrize("radius", RADII)
def test_luma_moves_by_at_most_one_code(rng, radius):
    """77 dr + 150 dg + 29 db is within 150 / 2 + |x| (150 * 437 / 65536 - 1) of 0, so the weighted sum moves by less than
    256: the luma by at most one code wherever no channel saturates."""
    for img in (S.scene_u8(rng, 40, 52), rng.integers(0, 256, (21, 33, 3)).astype(np.uint8)):
        for tl, tc, strength in ((8, 12, 1.0), (255, 255, 1.0), (40, 60, 0.7)):
            out = C.chroma_denoise_rgb(img, radius, tl, tc, strength)
            assert not np.array_equal(out, img)
            d = out.astype(np.int64) - img
            exact = np.repeat(np.repeat(np.stack(C.deltas(*C.cells_rgb(img), radius, tl, tc, strength), -1), 2, 0), 2, 1)
            exact = exact[:img.shape[0], :img.shape[1]][..., [1, 2, 0]]                 # (db, dr, dg) -> (dr, dg, db)
            free = (d == exact).all(axis=2)                                             # no channel saturated
            assert free.mean() > 0.5
            assert np.abs(S.luma(out) - S.luma(img))[free].max() <= 1


@pytest.mark.parametrize("radius", RADII)
def test_the_operator_commutes_with_the_transpose(rng, radius):
    for H, W in ((1, 1), (1, 6), (5, 1), (7, 10), (9, 9), (12, 5), (16, 22)):
        img = S.scene_u8(rng, H, W, sigma=0.06)
        for tl, tc, strength in ((8, 12, 1.0), (255, 255, 0.5)):
            a = O.transform(C.chroma_denoise_rgb(img, radius, tl, tc, strength), "transpose")
            b = C.chroma_denoise_rgb(np.ascontiguousarray(O.transform(img, "transpose")), radius, tl, tc, strength)
            assert np.array_equal(a, b), (H, W)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", TRANSFORMS)
def test_the_operator_commutes_with_the_transforms_on_even_sizes(rng, radius, name):
    for H, W in ((16, 16),) if name == "transverse" else ((16, 16), (10, 14), (2, 6)):
        img = S.scene_u8(rng, H, W, sigma=0.06)
        a = O.transform(C.chroma_denoise_rgb(img, radius, 8, 12, 1.0), name)
        b = C.chroma_denoise_rgb(np.ascontiguousarray(O.transform(img, name)), radius, 8, 12, 1.0)
        assert np.array_equal(a, b), (name, H, W)


def test_a_flip_along_an_odd_axis_does_not_commute(rng):
    """The cell grid is anchored at (0, 0) of the image: flipping 15 columns pairs other columns into cells."""
    img = S.scene_u8(rng, 16, 15, sigma=0.06)
    a = O.transform(C.chroma_denoise_rgb(img, 2, 8, 12, 1.0), "flip_horiz")
    b = C.chroma_denoise_rgb(np.ascontiguousarray(O.transform(img, "flip_horiz")), 2, 8, 12, 1.0)
    assert not np.array_equal(a, b)


def test_the_inputs_of_the_gpu_tests_are_not_vacuous(rng):
    """What tests/test_gpu_chroma_denoise.py relies on.  On uniform random bytes the thresholded settings leave most cells
    alone with n = 1 (74 % of them at radius 3 with (8, 12), 99.8 % at radius 1 with (8, 3)), so the output is mostly the
    input: random bytes go with (255, 255) only.  On the scene the thresholded settings keep 1 < n < (2r + 1)^2, the
    windows in which the tests decide, on a good part of the cells from 30 x 30 up: 0.30 of them at the least (radius 1,
    (8, 3), 31 x 33; the test asks for a quarter), about half or more at radius 2 and 3, 0.8 and more with (8, 12); the
    same on the planar scene."""
    noise = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    for r in RADII:
        full = (2 * r + 1) ** 2
        for tl, tc in ((8, 12), (2, 12), (8, 3)):
            n, _, _ = C.window(*C.cells_rgb(noise), r, tl, tc)
            assert (n == 1).mean() >= 0.7, (r, tl, tc)
            for H, W in ((30, 30), (31, 33), (64, 64), (70, 131)):
                n, _, _ = C.window(*C.cells_rgb(S.scene_u8(rng, H, W)), r, tl, tc)
                assert ((n > 1) & (n < full)).mean() >= 0.25, (r, tl, tc, H, W)
            for H, W in ((30, 34), (64, 96)):
                n, _, _ = C.window(*C.cells_yuv420(C.scene_yuv420(rng, H, W)), r, tl, tc)
                assert ((n > 1) & (n < full)).mean() >= 0.25, ("yuv", r, tl, tc, H, W)


def test_scene_yuv420_layout(rng):
    yuv = C.scene_yuv420(np.random.default_rng(5), 8, 12)
    rgb = S.scene_u8(np.random.default_rng(5), 8, 12).astype(np.float64)
    assert yuv.shape == (12, 12) and yuv.dtype == np.uint8
    y = np.rint(rgb @ np.array([0.299, 0.587, 0.114]))
    assert np.array_equal(yuv[:8], y.astype(np.uint8))
    u = (rgb @ np.array([-0.168736, -0.331264, 0.5]) + 128.0).reshape(4, 2, 6, 2).mean(axis=(1, 3))
    assert np.array_equal(yuv[8:].reshape(2, 4, 6)[0], np.rint(u).astype(np.uint8))
    assert C.scene_yuv420(rng, 2, 2).shape == (3, 2)


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_chroma_denoise_settings():
    s = ChromaDenoise()
    assert (s.radius, s.luma_threshold, s.chroma_threshold, s.strength) == (2, 8, 12, 1.0) and s.strength_q6 == 64
    assert ChromaDenoise(strength=0.5).strength_q6 == 32 and ChromaDenoise(strength=0).strength_q6 == 0
    assert ChromaDenoise(strength=0.0078125).strength_q6 == 1 and ChromaDenoise(strength=0.0078).strength_q6 == 0
    assert [ChromaDenoise(strength=a).strength_q6 for a in (0.3, 0.7, 1.0)] == [C.strength_q6(a) for a in (0.3, 0.7, 1.0)]
    assert ChromaDenoise(3, 255, 255, 1).radius == 3 and ChromaDenoise(1, 0, 0, 0.25).luma_threshold == 0
    assert check_chroma_denoise(None) is None and check_chroma_denoise(s) is s
    a = ChromaDenoise(3, 5, 7, 0.5)._arg()
    assert (a.radius, a.luma_threshold, a.chroma_threshold, a.strength_q6) == (3, 5, 7, 32)
    for bad in ({"radius": 0}, {"radius": 4}, {"radius": 1.0}, {"radius": True}, {"radius": None},
                {"luma_threshold": -1}, {"luma_threshold": 256}, {"luma_threshold": 8.0}, {"luma_threshold": True},
                {"luma_threshold": None}, {"chroma_threshold": -1}, {"chroma_threshold": 256}, {"chroma_threshold": 12.0},
                {"chroma_threshold": False}, {"strength": -0.1}, {"strength": 1.01}, {"strength": math.inf},
                {"strength": math.nan}, {"strength": "1"}, {"strength": True}, {"strength": None}):
        with pytest.raises(ValueError):
            ChromaDenoise(**bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.strength = 0.5
    for bad in (True, 1, 0.5, (2, 8, 12), "on"):
        with pytest.raises(ValueError):
            check_chroma_denoise(bad)
    with pytest.raises(ValueError):
        camera_isp.Camera16(camera_isp.bayer.BayerPattern.RGGB, chroma_denoise=1.0)


def test_package_exports_chroma_denoise():
    import taichi_image_amd as ti
    assert ti.ChromaDenoise is ChromaDenoise
    assert ti.chroma_denoise.chroma_denoise and ti.chroma_denoise.chroma_denoise_yuv420 and ti.chroma_denoise.apply


def test_chroma_denoise_entry_points_validate_on_the_host():
    """Every bad setting, count, shape and pointer is refused before anything is launched (no device)."""
    from taichi_image_amd import _native
    assert {"mi_isp_chroma_denoise_rgb_batch", "mi_isp_chroma_denoise_yuv420_batch"} <= set(_native.SIGNATURES)
    L = _native.lib()
    good = _native.ChromaDenoise(2, 8, 12, 64)
    src = (ctypes.c_void_p * 2)(0x1000, 0x3000)
    dst = (ctypes.c_void_p * 2)(0x2000, 0x4000)

    def refused(rc):
        assert rc == 1                                           # (1: a host check; 2 would be a launch error)
        assert b"chroma_denoise" in L.mi_isp_last_error()

    for fn in (L.mi_isp_chroma_denoise_rgb_batch, L.mi_isp_chroma_denoise_yuv420_batch):
        for s in (_native.ChromaDenoise(0, 8, 12, 64), _native.ChromaDenoise(4, 8, 12, 64), _native.ChromaDenoise(2, -1, 12, 64),
                  _native.ChromaDenoise(2, 256, 12, 64), _native.ChromaDenoise(2, 8, -1, 64), _native.ChromaDenoise(2, 8, 256, 64),
                  _native.ChromaDenoise(2, 8, 12, -1), _native.ChromaDenoise(2, 8, 12, 65)):
            refused(fn(src, dst, 2, 8, 8, s, None))
        refused(fn(src, dst, 2, 8, 8, None, None))
        refused(fn(src, dst, -1, 8, 8, good, None))
        refused(fn(src, dst, 2, -2, 8, good, None))
        refused(fn(src, dst, 2, 8, -2, good, None))
        refused(fn(None, dst, 2, 8, 8, good, None))
        refused(fn(src, None, 2, 8, 8, good, None))
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, 0x3000), 2, 8, 8, good, None))     # image 1 in place
        refused(fn(src, (ctypes.c_void_p * 2)(0x2000, None), 2, 8, 8, good, None))
        assert fn(src, dst, 0, 8, 8, good, None) == 0            # n == 0 and H * W == 0: successful no-ops
        assert fn(src, dst, 2, 0, 8, good, None) == 0
        assert fn(src, dst, 2, 8, 0, good, None) == 0
    refused(L.mi_isp_chroma_denoise_yuv420_batch(src, dst, 2, 7, 8, good, None))          # odd Y plane sides
    refused(L.mi_isp_chroma_denoise_yuv420_batch(src, dst, 2, 8, 7, good, None))


def test_scan_cli_takes_the_settings():
    from taichi_image_amd.scripts import tonemap_scan
    a = tonemap_scan.build_parser().parse_args(["--images", "x", "--chroma-denoise", "0.5", "--chroma-denoise-radius", "3",
                                                "--chroma-denoise-thresholds", "4", "9"])
    assert (a.chroma_denoise, a.chroma_denoise_radius, a.chroma_denoise_thresholds) == (0.5, 3, [4, 9])
    d = tonemap_scan.build_parser().parse_args(["--images", "x"])
    assert (d.chroma_denoise, d.chroma_denoise_radius, d.chroma_denoise_thresholds) == (None, None, None)
    for bad in (["--chroma-denoise", "1.5"], ["--chroma-denoise", "-1"], ["--chroma-denoise", "1", "--chroma-denoise-radius", "4"],
                ["--chroma-denoise", "1", "--chroma-denoise-thresholds", "256", "12"],
                ["--chroma-denoise", "1", "--chroma-denoise-thresholds", "8", "-1"],
                ["--chroma-denoise-radius", "2"], ["--chroma-denoise-thresholds", "8", "12"]):   # (the last two: no STRENGTH)
        with pytest.raises(ValueError):                          # refused before any frame is read
            tonemap_scan.main(["--images", "/nonexistent"] + bad)


# ---- the kernel's division ---------------------------------------------------------------------------------------------
def test_the_kernels_division_is_floor_division():
    """cdn::floor_div_512n of csrc/isp_chroma_denoise.h, compiled for the host, against floor division for every n in
    1 .. 49 and every numerator in [-(2^24 + 256 * 49), 2^24 + 256 * 49] (tests/check_chroma_denoise_div.cpp)."""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "check")
        subprocess.run(["g++", "-O2", "-fopenmp", "-ffp-contract=off", os.path.join(here, "check_chroma_denoise_div.cpp"),
                        "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "FAIL" not in out.stdout and out.stdout.count("ok") == 50, out.stdout
