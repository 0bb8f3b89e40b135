"""The antialiased resize without a GPU ("Antialiased resize"): the library's host-built tables against the
independent restatement of tests/resample_ref.py, hand vectors, the limits and host checks (made-up addresses: nothing is
launched or dereferenced), and properties of the restatement alone that pin the operator, not just its agreement with
itself."""
import ctypes

import numpy as np
import pytest
import torch

from taichi_image_amd import _native, interpolate, resample as rs
from taichi_image_amd import BayerPattern, Camera16, Camera32, LensDistortion, Resample
from tests import resample_ref as R

FILTERS = R.FILTERS
# (row scale, col scale): 1/8 is beyond lanczos3's limit; the last is the per-axis pair
SCALES = [(1 / 8, 1 / 8), (1 / 4, 1 / 4), (240 / 512, 240 / 512), (1.0, 1.0), (2.0, 2.0), (240 / 512, 0.75)]
SIZES = [1, 3, 10, 512]


def _axes():
    """(filter, S, D, scale) of every axis of the table tests."""
    out = []
    for f in FILTERS:
        for s0, s1 in SCALES:
            if f == "lanczos3" and min(s0, s1) == 1 / 8:
                continue
            for S in SIZES:
                for s in sorted({s0, s1}):
                    out.append((f, S, max(1, round(S * s)), s))
    return sorted(set(out))


def _ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("filt,S,D,s", _axes())
def test_table_matches_the_restatement(filt, S, D, s):
    T, start, weight = rs.table(filt, S, D, s)
    Tr, start_r, weight_r = R.table(filt, S, D, s)
    assert T == Tr == rs.taps(filt, S, D, s) and 1 <= T <= min(32, S)
    assert start.dtype == np.int32 and weight.dtype == np.float32 and weight.shape == (D, T)
    assert np.array_equal(start, start_r)
    if filt == "lanczos3":                   # (the C library and Python may differ in the last bit of sin)
        assert _ulp_distance(weight, weight_r).max() <= 1
    else:
        assert np.array_equal(weight.view(np.uint32), weight_r.view(np.uint32))
    assert np.all(np.abs(weight.astype(np.float64).sum(1) - 1.0) <= T * 2.0 ** -24)
    assert start.min() >= 0 and np.all(start + T <= S)


def test_tap_counts_of_the_headline_scales():
    s = 1920 / 4096
    assert [rs.taps(f, 4096, 1920, s) for f in FILTERS] == [4, 5, 13]
    assert [rs.taps(f, 4096, 512, 1 / 8) for f in ("area", "triangle")] == [9, 15]
    assert R.table("lanczos3", 4096, 512, 1 / 8, limit=False)[0] == 47


def test_hand_vector_area_half():
    T, start, weight = rs.table("area", 10, 5, 0.5)
    assert T == 3 and start.tolist() == [0, 1, 3, 5, 7]
    assert weight[0].tolist() == [0.75, 0.25, 0.0]
    for d in range(1, 5):
        assert weight[d].tolist() == [0.25, 0.5, 0.25]


@pytest.mark.parametrize("filt", ["area", "triangle"])
def test_hand_vector_scale_two_is_bilinear(filt):
    T, start, weight = rs.table(filt, 8, 16, 2.0)
    assert T == 2
    for d in range(14):                      # (the last two fold onto the edge sample)
        assert start[d] == d // 2 and weight[d].tolist() == ([1.0, 0.0] if d % 2 == 0 else [0.5, 0.5])
    assert start[14:].tolist() == [6, 6] and weight[14].tolist() == [0.0, 1.0] and weight[15].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("filt", FILTERS)
def test_scale_one_is_the_identity(filt):
    T, start, weight = rs.table(filt, 37, 37, 1.0)
    assert T == 1 and start.tolist() == list(range(37)) and np.all(weight == 1.0)


def test_limits():
    with pytest.raises(ValueError, match=r"lanczos3.*0\.125.*0\.1875"):
        rs.taps("lanczos3", 4096, 512, 1 / 8)
    with pytest.raises(ValueError, match="lanczos3"):
        rs.table("lanczos3", 4096, 512, 1 / 8)
    with pytest.raises(ValueError, match=r"triangle.*0\.0625"):
        rs.taps("triangle", 4096, 128, 1 / 32)
    assert rs.taps("triangle", 4096, 256, 1 / 16) == 31
    # T > S is capped: every tap folds onto the few samples there are
    T, start, weight = rs.table("lanczos3", 3, 2, 0.4)
    assert T == 3 and start.tolist() == [0, 0]
    assert rs.taps("lanczos3", 5, 1, 1 / 8) == 5 and rs.taps("area", 1, 1, 1 / 31) == 1
    for bad in ("cubic", "", None, 3):
        with pytest.raises(ValueError, match="must be one of"):
            rs.taps(bad, 8, 4, 0.5)
        with pytest.raises(ValueError, match="must be one of"):
            Resample(bad)
    with pytest.raises(ValueError, match="no table"):
        rs.taps("bilinear", 8, 4, 0.5)
    for S, D, s in ((0, 4, 0.5), (8, 0, 0.5), (8, 4, 0.0), (8, 4, -1.0), (8, 4, float("nan")), (8, 4, float("inf"))):
        with pytest.raises(ValueError):
            rs.taps("area", S, D, s)
    assert rs.check_resample(None) is None and rs.check_resample(Resample("triangle")).filter == "triangle"
    with pytest.raises(ValueError, match="must be None or a Resample"):
        rs.check_resample("area")
    assert rs.FILTERS == ("bilinear", "area", "triangle", "lanczos3") and Resample().filter == "area"


def test_integer_images_and_bad_calls_raise_before_anything_launches():
    for dt in (np.uint8, np.uint16):
        with pytest.raises(ValueError, match="f16 or f32"):
            interpolate.resample(np.zeros((8, 8, 3), dt), (4, 4))
    with pytest.raises(ValueError, match="f16 or f32"):
        interpolate.resample(np.zeros((8, 8, 3), np.float32), (4, 4), dtype="u8")
    with pytest.raises(ValueError, match="must be one of"):
        interpolate.resample(np.zeros((8, 8, 3), np.float32), (4, 4), filter="cubic")
    with pytest.raises(ValueError, match="lanczos3"):
        interpolate.resample(np.zeros((512, 512, 3), np.float32), (64, 64), filter="lanczos3")


_bufs = [(ctypes.c_uint8 * 4096)() for _ in range(4)]
_addr = [ctypes.addressof(b) for b in _bufs]


def _batch(L, **kw):
    a = dict(src=_addr[0], dst=_addr[1], n=1, Hs=8, Ws=8, Hd=4, Wd=4, ti=_native.MI_F16, to=_native.MI_F32,
             rows=_native.ResampleAxis(3, _addr[2], _addr[3]), cols=_native.ResampleAxis(3, _addr[2], _addr[3]))
    a.update(kw)
    p = lambda v: (ctypes.c_void_p * 1)(v)                            # noqa: E731  (None: a list holding a null)
    q = lambda t: None if t is None else ctypes.byref(t)             # noqa: E731
    rc = L.mi_isp_resample_batch(None if a["src"] == "nolist" else p(a["src"]), p(a["dst"]), a["n"], a["Hs"], a["Ws"],
                                 a["Hd"], a["Wd"], a["ti"], a["to"], q(a["rows"]), q(a["cols"]), None)
    return rc, L.mi_isp_last_error().decode()


@pytest.mark.parametrize("bad,text", [
    (dict(n=-1), "resample with -1 images"),
    (dict(Hs=0), "resample source 0 x 8"),
    (dict(Wd=-1), "resample output 4 x -1"),
    (dict(ti=_native.MI_U8), "resample takes MI_F16 / MI_F32"),
    (dict(to=_native.MI_U16), "resample takes MI_F16 / MI_F32"),
    (dict(rows=None), "null resample row table"),
    (dict(cols=_native.ResampleAxis(0, _addr[2], _addr[3])), "resample column table with 0 taps"),
    (dict(cols=_native.ResampleAxis(33, _addr[2], _addr[3]), Ws=64), "resample column table with 33 taps"),
    (dict(rows=_native.ResampleAxis(9, _addr[2], _addr[3])), "resample row table with 9 taps"),
    (dict(rows=_native.ResampleAxis(3, None, _addr[3])), "resample row table without starts or weights"),
    (dict(src=None), "resample image 0 has a null pointer"),
    (dict(src="nolist"), "null resample image list"),
    (dict(src=_addr[0] + 1), "resample image 0 not aligned"),
    (dict(dst=_addr[0]), "cannot run in place"),
])
def test_host_checks_run_before_any_launch(bad, text):
    rc, err = _batch(_native.lib(), **bad)
    assert rc == 1 and err.startswith("resample_batch: ") and text in err


def test_a_zero_sized_output_launches_nothing():
    L = _native.lib()
    assert _batch(L, Hd=0)[0] == 0 and _batch(L, Wd=0)[0] == 0 and _batch(L, n=0)[0] == 0


@pytest.mark.parametrize("Camera", [Camera16, Camera32])
def test_camera_option_is_checked_before_anything_launches(Camera):
    with pytest.raises(ValueError, match="must be None or a Resample"):
        Camera(BayerPattern.RGGB, resample="area")
    cam = Camera(BayerPattern.RGGB, resize_width=16, resample=Resample("area"))
    assert cam.resample == Resample("area")
    cam.set(resample=Resample("triangle"))
    assert cam.resample.filter == "triangle"
    cam.set(resample=False)
    assert cam.resample is None
    with pytest.raises(ValueError, match="must be None or a Resample"):
        cam.set(resample="area")
    cam.set(resample=Resample("lanczos3"))
    frame = torch.zeros((24, 48), dtype=torch.uint8)                  # a 24 x 32 packed-12 frame; 16 / 32 = 0.5
    # a table lens of the resize geometry (what the bilinear route takes) is not the frame's shape
    lens = LensDistortion.from_map(np.zeros((12, 16, 2), np.float32), (24, 32))
    with pytest.raises(ValueError, match="must have the frame's shape"):
        cam.load_packed12(frame, undistort=lens)
    with pytest.raises(ValueError, match="must have the frame's shape"):
        cam.load_16u(torch.zeros((24, 32), dtype=torch.uint16), undistort=lens)
    # a scale the filter does not take: 16 / 256 is below lanczos3's 3 / 16
    with pytest.raises(ValueError, match="lanczos3"):
        cam.load_packed12(torch.zeros((64, 384), dtype=torch.uint8))


def test_scan_cli_flag():
    from taichi_image_amd.scripts import tonemap_scan as ts
    ap = ts.build_parser()
    assert ap.parse_args(["--images", "x"]).resample is None
    for f in rs.FILTERS:
        assert ap.parse_args(["--images", "x", "--resample", f]).resample == f
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--resample", "cubic"])


# ---- reference-only properties: the 384 x 512 source at the config-3 ratio ------------------------------------------------
HS, WS, SCALE = 384, 512, 240 / 512
HD, WD = 180, 240


def _mono(plane):
    return np.repeat(plane.astype(np.float32)[:, :, None], 3, 2)


@pytest.fixture(scope="module")
def noise():
    return _mono(np.random.default_rng(7).standard_normal((HS, WS)))


def _cosine(period):
    """0.5 + 0.5 cos along the rows: std 0.354."""
    x = np.arange(WS)[None, :] + np.zeros((HS, 1))
    return _mono(0.5 + 0.5 * np.cos(2 * np.pi * x / period))


def test_white_noise_is_averaged(noise):
    for f in FILTERS:
        assert R.resize(noise, (WD, HD), SCALE, f)[..., 0].var() < 0.20, f
    assert R.bilinear(noise, (WD, HD), SCALE)[..., 0].var() > 0.40


def test_a_cosine_above_nyquist_is_removed():
    src = _cosine(2.2)
    for f in FILTERS:
        assert R.resize(src, (WD, HD), SCALE, f)[10:-10, 10:-10, 0].std() < 0.04, f
    assert R.bilinear(src, (WD, HD), SCALE)[10:-10, 10:-10, 0].std() > 0.15


def test_a_cosine_below_nyquist_is_kept():
    src = _cosine(16)                                                 # (the ideal std is 0.354)
    for f in FILTERS:
        assert R.resize(src, (WD, HD), SCALE, f)[10:-10, 10:-10, 0].std() > 0.32, f


@pytest.mark.parametrize("filt", FILTERS)
def test_a_constant_image_comes_back(filt):
    src = np.full((HS, WS, 3), 0.7231, np.float32)
    out = R.resize(src, (WD, HD), SCALE, filt)
    Ty, Tx = R.table(filt, HS, HD, SCALE)[0], R.table(filt, WS, WD, SCALE)[0]
    assert np.abs(out / np.float32(0.7231) - 1).max() <= 4 * (Tx + Ty) * 2.0 ** -24
