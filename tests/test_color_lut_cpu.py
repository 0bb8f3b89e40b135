"""The 3D colour LUT without a GPU: the NumPy statement of the contract (tests/color_lut_ref.py) pinned by hand and by the
properties DESIGN.md 3 lists, ColorLut's checks and its .cube reader, the C entry points' host checks, the kernel's division
helper against the division (a host program), and that what the GPU tests run is not vacuous."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from taichi_image_amd import camera_isp
from taichi_image_amd.color_lut import ColorLut, check_color_lut
from tests import color_lut_ref as C


def all_codes():
    """(256, 1, 3) image: code k in every channel, and the same codes shifted per channel."""
    k = np.arange(256, dtype=np.uint8)
    return np.stack([k, k[::-1], np.roll(k, 101)], -1).reshape(256, 1, 3)


# ---- the properties the contract lists -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", range(2, 66))
def test_the_identity_table_is_the_identity(N):
    """Each output channel of the identity table depends on its own input channel only, so all 256 codes per channel cover
    all 2^24 colours."""
    t = C.identity_table(N)
    assert np.array_equal(t, ColorLut.identity(N).table)
    img = all_codes()
    assert np.array_equal(C.color_lut_rgb(img, t), img)
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2)
    assert np.array_equal(C.color_lut_rgb(grey, t), grey)
    assert np.array_equal(C.color_lut_rgb(img, t, 0.5), img)


@pytest.mark.parametrize("N", [2, 3, 17, 33, 65])
def test_the_order_of_tied_fractions_does_not_matter(rng, N):
    """color_lut_rgb computes both orders and asserts that they agree; here on an image where most pixels tie."""
    ties = C.ties_and_ends_image()
    v = ties.reshape(-1, 3).astype(np.int64)
    f = (v * (N - 1)) % 255
    tied = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    assert tied.mean() > 0.5
    t = C.random_table(rng, N)
    a = C._interpolate(v, t, False, False, False, False)
    b = C._interpolate(v, t, True, False, False, False)
    assert np.array_equal(a, b)
    C.color_lut_rgb(ties, t)


def test_two_points_by_hand(rng):
    """N = 2: p = v, i = 0 below 255 and 1 at 255, f = v (0 at 255).  Every corner colour comes back as the table's own
    entry.  Mid-cube (200, 100, 50): f_R >= f_G >= f_B, so the corners are 000, 100, 110, 111 with weights 55, 100, 50, 50:
    y_c = (55 T000 + 100 T100 + 50 T110 + 50 T111 + 127) // 255."""
    t = C.random_table(rng, 2)
    for r in (0, 1):
        for g in (0, 1):
            for b in (0, 1):
                px = np.array([[[255 * r, 255 * g, 255 * b]]], np.uint8)
                assert np.array_equal(C.color_lut_rgb(px, t)[0, 0], t[r, g, b])
    T = t.astype(np.int64)
    want = (55 * T[0, 0, 0] + 100 * T[1, 0, 0] + 50 * T[1, 1, 0] + 50 * T[1, 1, 1] + 127) // 255
    assert np.array_equal(C.color_lut_rgb(np.array([[[200, 100, 50]]], np.uint8), t)[0, 0], want)
    # the same fractions on other axes: (50, 200, 100) orders G, B, R
    want = (55 * T[0, 0, 0] + 100 * T[0, 1, 0] + 50 * T[0, 1, 1] + 50 * T[1, 1, 1] + 127) // 255
    assert np.array_equal(C.color_lut_rgb(np.array([[[50, 200, 100]]], np.uint8), t)[0, 0], want)
    # fixed numbers: T000 = (10, 20, 30), T100 = (200, 0, 90), T110 = (250, 255, 1), T111 = (7, 128, 64)
    t2 = np.zeros((2, 2, 2, 3), np.uint8)
    t2[0, 0, 0], t2[1, 0, 0], t2[1, 1, 0], t2[1, 1, 1] = (10, 20, 30), (200, 0, 90), (250, 255, 1), (7, 128, 64)
    # R: 550 + 20000 + 12500 + 350 + 127 = 33527 // 255 = 131; G: 1100 + 0 + 12750 + 6400 + 127 = 20377 // 255 = 79;
    # B: 1650 + 9000 + 50 + 3200 + 127 = 14027 // 255 = 55.  Without the + 127: 33400 // 255 = 130, 20250 // 255 = 79,
    # 13900 // 255 = 54
    px = np.array([[[200, 100, 50]]], np.uint8)
    assert C.color_lut_rgb(px, t2)[0, 0].tolist() == [131, 79, 55]
    assert C.color_lut_rgb(px, t2, truncate=True)[0, 0].tolist() == [130, 79, 54]


def test_the_strength_rounding():
    """out = v + (((y - v) S + 32) >> 6) with an arithmetic shift, y - v of either sign.  A two-point table with constant
    colour (y = the colour everywhere)."""
    for y, v in ((200, 100), (100, 200), (101, 100), (100, 101), (0, 255), (255, 0), (130, 97), (97, 130)):
        t = np.full((2, 2, 2, 3), y, np.uint8)
        px = np.full((1, 1, 3), v, np.uint8)
        for S in (0, 1, 32, 64):
            want = v + (((y - v) * S + 32) >> 6)                    # (Python's >> is arithmetic)
            assert C.color_lut_rgb(px, t, S / 64)[0, 0].tolist() == [want] * 3, (y, v, S)
        assert C.color_lut_rgb(px, t, 0.0)[0, 0, 0] == v and C.color_lut_rgb(px, t, 1.0)[0, 0, 0] == y
    # by hand: y - v = -100, S = 1: (-100 + 32) >> 6 = -68 >> 6 = -2 (truncation toward zero would give -1)
    assert C.color_lut_rgb(np.full((1, 1, 3), 200, np.uint8), np.full((2, 2, 2, 3), 100, np.uint8), 1 / 64)[0, 0, 0] == 198
    # y - v = -33, S = 32: (-1056 + 32) >> 6 = -16; y - v = 33: (1056 + 32) >> 6 = 17
    assert C.color_lut_rgb(np.full((1, 1, 3), 130, np.uint8), np.full((2, 2, 2, 3), 97, np.uint8), 0.5)[0, 0, 0] == 114
    assert C.color_lut_rgb(np.full((1, 1, 3), 97, np.uint8), np.full((2, 2, 2, 3), 130, np.uint8), 0.5)[0, 0, 0] == 114


def test_the_division_constant_over_the_whole_range():
    x = np.arange(0, 65025 + 127 + 1, dtype=np.uint64)
    assert np.array_equal((x * 0x8081) >> 23, x // 255)
    assert int(x[-1]) * 0x8081 < 2 ** 32                            # the product fits the kernel's 32 bits


def test_the_kernels_division_is_the_division():
    """clut::div255 of csrc/isp_color_lut.h, compiled for the host, against x / 255 for every numerator of the contract
    (tests/check_color_lut_div.cpp)."""
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "check")
        subprocess.run(["g++", "-O2", os.path.join(here, "check_color_lut_div.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "FAIL" not in out.stdout and out.stdout.strip() == "ok 65153", out.stdout


def test_the_mutants_are_other_operators(rng):
    t = C.look_table(17)
    img = rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)
    ref = C.color_lut_rgb(img, t)
    assert not np.array_equal(ref, img)
    for kw in ({"trilinear": True}, {"truncate": True}, {"swap_axes": True}):
        assert not np.array_equal(ref, C.color_lut_rgb(img, t, **kw)), kw
    # on the grid points themselves (N = 16: codes 17 k, every fraction 0) both give the table's entry
    t = C.look_table(16)
    grid = (np.arange(16) * 17).astype(np.uint8)
    g = np.stack(np.meshgrid(grid, grid, grid, indexing="ij"), -1).reshape(-1, 1, 3)
    assert np.array_equal(C.color_lut_rgb(g, t), t.reshape(-1, 1, 3))
    assert np.array_equal(C.color_lut_rgb(g, t, trilinear=True), t.reshape(-1, 1, 3))


def test_the_inputs_of_the_gpu_tests_are_not_vacuous():
    """For every (table, image) pair tests/test_gpu_color_lut.py runs on at least 1000 pixels (the four smaller shapes are
    there for the byte path and the tails; a handful of pixels cannot tell a dropped + 127): the reference differs from
    its input and from each of the three mutants.  The identity table is the exception: it is there to be the identity."""
    for N in C.GPU_POINTS:
        tables = C.gpu_tables(N)
        for H, W in C.GPU_SHAPES:
            if H * W < 1000:
                continue
            for iname, img in C.gpu_images(H, W).items():
                assert np.array_equal(C.color_lut_rgb(img, tables["identity"]), img)
                for tname in ("random", "look"):
                    what = (N, H, W, iname, tname)
                    ref = C.color_lut_rgb(img, tables[tname])
                    assert not np.array_equal(ref, img), what
                    for kw in ({"trilinear": True}, {"truncate": True}, {"swap_axes": True}):
                        assert not np.array_equal(ref, C.color_lut_rgb(img, tables[tname], **kw)), (what, kw)
                    half = C.color_lut_rgb(img, tables[tname], 0.5)
                    assert not np.array_equal(half, ref) and not np.array_equal(half, img), what
                    assert not np.array_equal(C.color_lut_rgb(img, tables[tname], 1 / 64), img), what


# ---- ColorLut ----------------------------------------------------------------------------------------------------------
def test_color_lut_fields(rng):
    t = C.random_table(rng, 5)
    lut = ColorLut(t)
    assert lut.n_points == 5 and lut.strength == 1.0 and lut.strength_q6 == 64
    assert np.array_equal(lut.table, t) and lut.table is not t and not lut.table.flags.writeable
    t[0, 0, 0, 0] ^= 1                                             # (a copy)
    assert not np.array_equal(lut.table, t)
    with pytest.raises(ValueError):
        lut.table[0, 0, 0, 0] = 1
    assert ColorLut(t, 0.5).strength_q6 == 32 and ColorLut(t, 0).strength_q6 == 0
    assert ColorLut(t, 0.0078125).strength_q6 == 1 and ColorLut(t, 0.0078).strength_q6 == 0
    assert [ColorLut(t, a).strength_q6 for a in (0.3, 0.7, 1.0)] == [C.strength_q6(a) for a in (0.3, 0.7, 1.0)]
    a = ColorLut(t, 0.5)._arg()
    assert (a.n_points, a.strength_q6) == (5, 32)
    p = ColorLut(t).packed()
    assert p.dtype == np.uint32 and p.shape == (125,)
    assert p[(1 * 5 + 2) * 5 + 3] == int(t[1, 2, 3, 0]) | int(t[1, 2, 3, 1]) << 8 | int(t[1, 2, 3, 2]) << 16
    assert ColorLut(t) == ColorLut(t.copy()) and ColorLut(t) != ColorLut(t, 0.5)
    assert check_color_lut(None) is None and check_color_lut(lut) is lut
    for bad in (True, 1, 0.5, t, "x.cube"):
        with pytest.raises(ValueError):
            check_color_lut(bad)
    for bad in (t[:4], t[..., :2], t[0], t.astype(np.int32), np.zeros((1, 1, 1, 3), np.uint8), np.zeros((66, 66, 66, 3), np.uint8),
                t.tolist(), None):
        with pytest.raises(ValueError):
            ColorLut(bad)
    for bad in (-0.1, 1.01, math.inf, math.nan, "1", True, None):
        with pytest.raises(ValueError, match="strength"):
            ColorLut(t, bad)
    with pytest.raises(ValueError):
        camera_isp.Camera16(camera_isp.bayer.BayerPattern.RGGB, color_lut=1.0)
    for bad in (1, 66, 2.0, True, None):
        with pytest.raises(ValueError):
            ColorLut.identity(bad)


def test_float_tables_are_quantised_once_in_float64():
    """floor(clip(x, 0, 1) * 255 + 0.5): x.5 boundaries go up, values outside [0, 1] are clipped, non-finite ones refused."""
    x = np.zeros((2, 2, 2, 3), np.float64)
    x[0, 0, 0] = (0.5 / 255, 1.5 / 255, 127.5 / 255)
    x[0, 0, 1] = (np.nextafter(0.5 / 255, 0), np.nextafter(127.5 / 255, 0), 254.5 / 255)
    x[0, 1, 0] = (-0.3, 1.7, 1.0)
    x[1, 1, 1] = (0.25, 0.5, 0.75)
    t = ColorLut(x).table
    assert t[0, 0, 0].tolist() == [1, 2, 128]
    assert t[0, 0, 1].tolist() == [0, 127, 255]
    assert t[0, 1, 0].tolist() == [0, 255, 255]
    assert t[1, 1, 1].tolist() == [64, 128, 191]
    assert np.array_equal(ColorLut(x.astype(np.float32)).table[1, 1, 1], [64, 128, 191])
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 0, 1, 2] = bad
        with pytest.raises(ValueError):
            ColorLut(y)


def cube_text(table01, title=True, domain=True, extra=()):
    """The .cube text of an (N, N, N, 3) float table indexed [r][g][b]: R varies fastest."""
    n = table01.shape[0]
    lines = ["# a comment", ""]
    if title:
        lines.append('TITLE "a look"')
    lines.append(f"LUT_3D_SIZE {n}")
    if domain:
        lines += ["DOMAIN_MIN 0.0 0.0 0.0", "DOMAIN_MAX 1.0 1.0 1.0", "LUT_3D_INPUT_RANGE 0.0 1.0"]
    lines += list(extra) + [""]
    for b in range(n):
        for g in range(n):
            for r in range(n):
                lines.append(" ".join(repr(float(x)) for x in table01[r, g, b]))
    return "\n".join(lines) + "\n"


def test_from_cube_round_trip(rng, tmp_path):
    t = C.random_table(rng, 4)
    text = cube_text(t / 255.0)
    lut = ColorLut.from_cube(text, 0.5)
    assert np.array_equal(lut.table, t) and lut.strength_q6 == 32
    path = tmp_path / "look.cube"
    path.write_text(text)
    assert ColorLut.from_cube(path) == ColorLut(t) and ColorLut.from_cube(str(path)) == ColorLut(t)
    assert ColorLut.from_cube(cube_text(t / 255.0, title=False, domain=False)) == ColorLut(t)
    assert ColorLut.from_cube(cube_text(t / 255.0).replace("\n", "\r\n")) == ColorLut(t)
    # the axis order: the second row is r = 1
    x = np.zeros((2, 2, 2, 3))
    x[1, 0, 0] = (1.0, 0.5, 0.0)
    assert ColorLut.from_cube(cube_text(x)).table[1, 0, 0].tolist() == [255, 128, 0]
    # quantisation at x.5 boundaries, as for a float table
    x[0, 1, 1] = (0.5 / 255, 127.5 / 255, np.nextafter(127.5 / 255, 0))
    assert ColorLut.from_cube(cube_text(x)).table[0, 1, 1].tolist() == [1, 128, 127]
    assert ColorLut.from_cube(cube_text(C.identity_table(17) / 255.0)) == ColorLut.identity(17)


def test_from_cube_errors(rng):
    t = C.random_table(rng, 2) / 255.0
    good = cube_text(t)
    ColorLut.from_cube(good)
    rows = good.splitlines()
    bad_texts = {
        "another domain min": good.replace("DOMAIN_MIN 0.0 0.0 0.0", "DOMAIN_MIN 0.1 0.0 0.0"),
        "another domain max": good.replace("DOMAIN_MAX 1.0 1.0 1.0", "DOMAIN_MAX 1.0 2.0 1.0"),
        "another input range": good.replace("LUT_3D_INPUT_RANGE 0.0 1.0", "LUT_3D_INPUT_RANGE 0.0 1023.0"),
        "a short domain": good.replace("DOMAIN_MAX 1.0 1.0 1.0", "DOMAIN_MAX 1.0 1.0"),
        "a 1D table": good.replace("LUT_3D_SIZE 2", "LUT_1D_SIZE 2"),
        "both sizes": good.replace("LUT_3D_SIZE 2", "LUT_3D_SIZE 2\nLUT_1D_SIZE 2"),
        "a row short": "\n".join(rows[:-1]) + "\n",
        "a row too many": good + "0.0 0.0 0.0\n",
        "two fields": "\n".join(rows[:-1] + ["0.5 0.5"]) + "\n",
        "four fields": "\n".join(rows[:-1] + ["0.5 0.5 0.5 0.5"]) + "\n",
        "not a number": "\n".join(rows[:-1] + ["0.5 x 0.5"]) + "\n",
        "nan": "\n".join(rows[:-1] + ["0.5 nan 0.5"]) + "\n",
        "inf": "\n".join(rows[:-1] + ["inf 0.5 0.5"]) + "\n",
        "an unknown keyword": good.replace("LUT_3D_SIZE 2", "LUT_3D_SIZE 2\nLUT_SHAPER 3"),
        "no size": good.replace("LUT_3D_SIZE 2\n", ""),
        "a size that is no integer": good.replace("LUT_3D_SIZE 2", "LUT_3D_SIZE 2.0"),
        "two sizes": good.replace("LUT_3D_SIZE 2", "LUT_3D_SIZE 2\nLUT_3D_SIZE 2"),
        "N = 1": "LUT_3D_SIZE 1\n0 0 0\n",
        "N = 66": "LUT_3D_SIZE 66\n" + "0 0 0\n" * 8,
    }
    for what, text in bad_texts.items():
        with pytest.raises(ValueError):
            ColorLut.from_cube(text)
            pytest.fail(what)
    with pytest.raises(ValueError):
        ColorLut.from_cube(good, 1.5)
    with pytest.raises(ValueError):
        ColorLut.from_cube(17)
    with pytest.raises(OSError):
        ColorLut.from_cube("/nonexistent/look.cube")


def test_package_exports_color_lut():
    import taichi_image_amd as ti
    assert ti.ColorLut is ColorLut
    assert ti.color_lut.apply_lut and ti.color_lut.apply and ti.color_lut.check_color_lut


def test_apply_lut_refuses_other_images_before_the_device(rng):
    from taichi_image_amd.color_lut import apply_lut
    lut = ColorLut.identity(2)
    img = rng.integers(0, 256, (4, 4, 3)).astype(np.uint8)
    for bad in (img.astype(np.float32), img.astype(np.uint16), img[..., :2], img[0], img[None], [1, 2, 3]):
        with pytest.raises(ValueError):
            apply_lut(bad, lut)
    with pytest.raises(ValueError):
        apply_lut(img, C.identity_table(2))


def test_color_lut_entry_points_validate_on_the_host():
    """Every bad setting, count, shape and pointer is refused before anything is launched (no device)."""
    from taichi_image_amd import _native
    assert {"mi_isp_color_lut_rgb_batch", "mi_isp_color_lut_rgb_batch_path"} <= set(_native.SIGNATURES)
    L = _native.lib()
    good = _native.ColorLut(17, 64)
    src = (ctypes.c_void_p * 2)(0x1000, 0x3000)
    dst = (ctypes.c_void_p * 2)(0x2000, 0x4000)
    table = ctypes.c_void_p(0x8000)

    def refused(rc):
        assert rc == 1                                           # (1: a host check; 2 would be a launch error)
        assert b"color_lut" in L.mi_isp_last_error()

    def both(src, dst, n, H, W, table, s):
        yield L.mi_isp_color_lut_rgb_batch(src, dst, n, H, W, table, s, None)
        yield L.mi_isp_color_lut_rgb_batch_path(src, dst, n, H, W, table, s, 0, None)

    for s in (_native.ColorLut(1, 64), _native.ColorLut(66, 64), _native.ColorLut(0, 64), _native.ColorLut(-3, 64),
              _native.ColorLut(17, -1), _native.ColorLut(17, 65), None):
        for rc in both(src, dst, 2, 8, 8, table, s):
            refused(rc)
    for args in ((src, dst, -1, 8, 8, table, good), (src, dst, 2, -2, 8, table, good), (src, dst, 2, 8, -2, table, good),
                 (None, dst, 2, 8, 8, table, good), (src, None, 2, 8, 8, table, good), (src, dst, 2, 8, 8, None, good),
                 (src, (ctypes.c_void_p * 2)(0x2000, None), 2, 8, 8, table, good),
                 ((ctypes.c_void_p * 2)(None, 0x3000), dst, 2, 8, 8, table, good)):
        for rc in both(*args):
            refused(rc)
    for path, s in ((3, good), (-1, good), (1, _native.ColorLut(34, 64)), (1, _native.ColorLut(65, 64))):
        refused(L.mi_isp_color_lut_rgb_batch_path(src, dst, 2, 8, 8, table, s, path, None))
    for n, H, W in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):            # n == 0 and H * W == 0: successful no-ops
        for rc in both(src, dst, n, H, W, table, good):
            assert rc == 0
