"""Lens distortion correction (lens.LensDistortion, interpolate.undistort / remap, undistort= of the raw loaders): the
host side, without a device.

contract_map and contract_remap restate the contract of DESIGN.md 3 ("Lens distortion") in NumPy f32 - every step one f32
operation, left to right - independently of lens.distortion_map; the GPU tests (tests/test_gpu_lens.py) hold the kernels
to them bit for bit.  opencv_map is OpenCV's published model in float64, the yardstick of the f32 arithmetic.
"""
import ctypes

import numpy as np
import pytest

from oracle import isp_oracle as O

f32 = np.float32

# realistic calibrations: (K, dist) of a 4096 x 3072 sensor; |k1| <= 0.4, the rational model included
K4K = np.array([[2900.0, 0.0, 2051.3], [0.0, 2893.5, 1529.8], [0.0, 0.0, 1.0]])
LENSES_4K = [
    (K4K, (-0.31, 0.12, 0.0011, -0.0007)),
    (K4K, (-0.28, 0.09, -0.0006, 0.0013, -0.021)),
    (K4K, (0.4, -0.25, 0.0009, 0.0004, 0.05)),
    (K4K, (-0.38, 0.2, 0.0008, -0.0012, -0.06, 0.02, 0.01, -0.004)),        # rational
    (K4K, (2.1, 0.9, -0.0011, 0.0006, 0.04, 2.4, 1.3, 0.11)),               # rational, OpenCV-style large terms
]


def contract_map(K, dist, Hd, Wd, scale=(1.0, 1.0), new_K=None):
    """(Hd, Wd, 2) f32 (us, vs) of DESIGN.md 3: u = f32(c) / s1, v = f32(r) / s0, x = (u - cx') * ifx', ...; the
    parameters rounded once from double, ifx' = f32(1 / fx') from double."""
    nK = K if new_K is None else new_K
    fx, fy, cx, cy = (f32(v) for v in (K[0][0], K[1][1], K[0][2], K[1][2]))
    ncx, ncy = f32(nK[0][2]), f32(nK[1][2])
    ifx, ify = f32(1.0 / float(nK[0][0])), f32(1.0 / float(nK[1][1]))
    d = [f32(v) for v in dist] + [f32(0.0)] * (8 - len(dist))
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    s0, s1 = f32(scale[0]), f32(scale[1])
    c = np.broadcast_to(np.arange(Wd, dtype=np.int32).astype(f32)[None, :], (Hd, Wd))
    r = np.broadcast_to(np.arange(Hd, dtype=np.int32).astype(f32)[:, None], (Hd, Wd))
    u = c / s1
    v = r / s0
    x = (u - ncx) * ifx
    y = (v - ncy) * ify
    r2 = x * x + y * y
    num = f32(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
    radial = num / (f32(1) + r2 * (k4 + r2 * (k5 + r2 * k6))) if len(dist) == 8 else num
    xd = x * radial + f32(2) * p1 * x * y + p2 * (r2 + f32(2) * x * x)
    yd = y * radial + p1 * (r2 + f32(2) * y * y) + f32(2) * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=-1).astype(f32)


def contract_remap(src, map_xy, border="constant", out_dtype=None):
    """The sampling rule of DESIGN.md 3 on an (H, W, 3) image: constant border 0 outside [0, H-1] x [0, W-1] or NaN, or
    the coordinates clamped (NaN to 0); taps floor, floor + 1 clamped; rows mixed first, then columns, * intensity,
    cast_out - O.resize_bilinear's arithmetic."""
    in_dtype = O.dtype_name(src)
    out_dtype = in_dtype if out_dtype is None else out_dtype
    H, W = src.shape[:2]
    us, vs = map_xy[..., 0].astype(f32), map_xy[..., 1].astype(f32)
    hm, wm = f32(H - 1), f32(W - 1)
    with np.errstate(invalid="ignore"):
        inside = (vs >= 0) & (vs <= hm) & (us >= 0) & (us <= wm)
    if border == "replicate":
        vs = np.minimum(np.maximum(np.nan_to_num(vs, nan=0.0), f32(0)), hm)
        us = np.minimum(np.maximum(np.nan_to_num(us, nan=0.0), f32(0)), wm)
        inside = np.ones_like(inside)
    else:
        vs, us = np.where(inside, vs, f32(0)), np.where(inside, us, f32(0))
    i, j = vs.astype(np.int64), us.astype(np.int64)                        # floor (>= 0)
    fr, fc = (vs - i.astype(f32))[..., None], (us - j.astype(f32))[..., None]
    i1, j1 = np.minimum(i + 1, H - 1), np.minimum(j + 1, W - 1)
    s = src.astype(f32)
    one = f32(1)
    y1 = s[i, j] * (one - fr) + s[i1, j] * fr
    y2 = s[i, j1] * (one - fr) + s[i1, j1] * fr
    out = (y1 * (one - fc) + y2 * fc) * f32(O.SCALE[out_dtype] / O.SCALE[in_dtype])
    out = np.where(inside[..., None], out, f32(0))
    return O.cast_out(out, out_dtype)


def opencv_map(K, dist, Hd, Wd, scale=(1.0, 1.0), new_K=None):
    """OpenCV's model in float64 (x = (u - cx') / fx', radial (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4 +
    k6 r^6), tangential 2 p1 x y + p2 (r^2 + 2 x^2), p1 (r^2 + 2 y^2) + 2 p2 x y)."""
    nK = K if new_K is None else new_K
    d = list(dist) + [0.0] * (8 - len(dist))
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    u = np.arange(Wd, dtype=np.float64)[None, :] / scale[1]
    v = np.arange(Hd, dtype=np.float64)[:, None] / scale[0]
    x = (u - nK[0][2]) / nK[0][0]
    y = (v - nK[1][2]) / nK[1][1]
    r2 = x * x + y * y
    radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([K[0][0] * xd + K[0][2], K[1][1] * yd + K[1][2]], axis=-1)


# ---- the calibration object ---------------------------------------------------------------------------------------------
def test_lens_validation():
    from taichi_image_amd.lens import LensDistortion
    good = (K4K, (0.1, 0.01, 0.0, 0.0))
    LensDistortion(*good, (3072, 4096))
    LensDistortion(*good, (3072, 4096), new_K=K4K * [[0.9], [0.9], [1]], border="replicate")
    skew = K4K.copy(); skew[0, 1] = 0.5
    bottom = K4K.copy(); bottom[2, 2] = 2.0
    neg = K4K.copy(); neg[1, 1] = -1.0
    zero = K4K.copy(); zero[0, 0] = 0.0
    inf = K4K.copy(); inf[0, 2] = np.inf
    nan = K4K.copy(); nan[1, 2] = np.nan
    big = K4K.copy(); big[0, 2] = 1e39                                    # finite in double, not in f32
    for K in (skew, bottom, neg, zero, inf, nan, big, K4K[:2], np.eye(4), np.array([["a"] * 3] * 3), K4K.astype(bool)):
        with pytest.raises(ValueError):
            LensDistortion(K, good[1], (3072, 4096))
        with pytest.raises(ValueError):
            LensDistortion(K4K, good[1], (3072, 4096), new_K=K)
    for d in ((0.1,), (0.1, 0.2, 0.3), (0.1,) * 6, (0.1,) * 7, (0.1,) * 9, (0.1, np.nan, 0, 0), (0.1, 0, np.inf, 0),
              (1e40, 0, 0, 0), np.zeros((2, 4)), ("a", "b", "c", "d"), np.ones(4, bool)):
        with pytest.raises(ValueError):
            LensDistortion(K4K, d, (3072, 4096))
    for shape in ((0, 4), (4, -2), (4,), (4, 4, 3), (4.0, 4), (True, 4), "44"):
        with pytest.raises(ValueError):
            LensDistortion(*good, shape)
    with pytest.raises(ValueError):
        LensDistortion(*good, (8, 8), border="wrap")
    assert LensDistortion(K4K, np.array([[0.1, 0.2, 0.0, 0.0, 0.3]]), (8, 8)).dist == (0.1, 0.2, 0.0, 0.0, 0.3)


def test_table_validation():
    from taichi_image_amd.lens import LensDistortion
    m = np.zeros((6, 8, 2), f32)
    lens = LensDistortion.from_map(m, (10, 12))
    assert lens.is_table and lens.table_shape == (6, 8) and lens.shape == (10, 12)
    m[0, 0] = 5.0                                                          # copied: later writes do not reach it
    assert lens.table[0, 0, 0] == 0.0 and not lens.table.flags.writeable
    for bad in (np.zeros((6, 8, 2), np.float64), np.zeros((6, 8, 2), np.float16), np.zeros((6, 8, 3), f32),
                np.zeros((6, 8), f32), np.zeros((6, 8, 1, 2), f32), np.zeros((0, 8, 2), f32), np.zeros((6, 8, 2), np.int32)):
        with pytest.raises(ValueError):
            LensDistortion.from_map(bad, (10, 12))
    with pytest.raises(ValueError):
        LensDistortion.from_map(np.zeros((6, 8, 2), f32), (10, 12), border="reflect")
    with pytest.raises(ValueError):
        LensDistortion.from_map(np.zeros((6, 8, 2), f32), (0, 12))


def test_check_lens():
    from taichi_image_amd.lens import LensDistortion, check_lens
    lens = LensDistortion(K4K, (0.1, 0.0, 0.0, 0.0), (30, 40))
    assert check_lens(None, (30, 40)) is None and check_lens(lens, (30, 40)) is lens
    with pytest.raises(ValueError):
        check_lens(lens, (30, 42))
    with pytest.raises(ValueError):
        check_lens("lens", (30, 40))
    table = LensDistortion.from_map(np.zeros((15, 20, 2), f32), (30, 40))
    assert check_lens(table, (30, 40), (15, 20)) is table
    with pytest.raises(ValueError):
        check_lens(table, (30, 40), (30, 40))


# ---- the f32 contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(LENSES_4K)))
def test_contract_matches_opencv_in_float64(k):
    """The f32 arithmetic stays within 1e-3 px of OpenCV's float64 model over a whole 4096 x 3072 frame (the pixels whose
    source lies within a frame's width of the sensor: the rest is sampled as border anyway)."""
    K, dist = LENSES_4K[k]
    got = contract_map(K, dist, 3072, 4096)
    ref = opencv_map(K, dist, 3072, 4096)
    near = np.all(np.abs(ref - [2048, 1536]) < [4096, 3072], axis=-1)
    assert near.mean() > 0.9
    err = np.abs(got.astype(np.float64) - ref)[near]
    assert err.max() <= 1e-3, f"max {err.max():.3e} px"


def test_contract_with_new_K_and_scale_matches_opencv():
    K, dist = LENSES_4K[3]
    nK = np.array([[2600.0, 0.0, 2040.0], [0.0, 2600.0, 1530.0], [0.0, 0.0, 1.0]])
    s = 1920 / 4096
    got = contract_map(K, dist, 1440, 1920, (s, s), nK)
    ref = opencv_map(K, dist, 1440, 1920, (float(f32(s)), float(f32(s))), nK)
    assert np.abs(got - ref).max() <= 1e-3


@pytest.mark.parametrize("k", range(len(LENSES_4K)))
def test_distortion_map_is_the_contract(k):
    """lens.distortion_map and this file's statement of the contract agree bit for bit."""
    from taichi_image_amd.lens import LensDistortion
    K, dist = LENSES_4K[k]
    lens = LensDistortion(K, dist, (3072, 4096))
    assert np.array_equal(lens.distortion_map(3072, 4096).view(np.uint32), contract_map(K, dist, 3072, 4096).view(np.uint32))
    nK = K * [[0.8], [0.85], [1]]
    lens = LensDistortion(K, dist, (3072, 4096), new_K=nK)
    got = lens.distortion_map(1440, 1920, (0.46875, 0.46875))
    assert np.array_equal(got.view(np.uint32), contract_map(K, dist, 1440, 1920, (0.46875, 0.46875), nK).view(np.uint32))


def test_identity_lens_is_the_identity_map():
    from taichi_image_amd.lens import LensDistortion
    K = np.array([[500.0, 0, 99.5], [0, 480.0, 75.25], [0, 0, 1]])
    m = LensDistortion(K, (0.0, 0.0, 0.0, 0.0), (150, 200)).distortion_map(150, 200)
    c, r = np.meshgrid(np.arange(200), np.arange(150))
    assert np.abs(m[..., 0] - c).max() < 1e-4 and np.abs(m[..., 1] - r).max() < 1e-4


def test_contract_remap_of_the_identity_table_is_the_image(rng):
    src = rng.random((7, 9, 3), dtype=f32)
    c, r = np.meshgrid(np.arange(9, dtype=f32), np.arange(7, dtype=f32))
    table = np.stack([c, r], -1)
    assert np.array_equal(contract_remap(src, table), src)
    assert np.array_equal(contract_remap(src, table, "replicate"), src)
    table[0, 0] = (-0.5, 0.0)
    table[1, 1] = (np.nan, 2.0)
    out = contract_remap(src, table)
    assert np.all(out[0, 0] == 0) and np.all(out[1, 1] == 0)
    rep = contract_remap(src, table, "replicate")
    assert np.array_equal(rep[0, 0], src[0, 0]) and np.array_equal(rep[1, 1], src[2, 0])


# ---- the C entry points ---------------------------------------------------------------------------------------------------
def _lens_arg(n_dist=4, border=0, **kw):
    from taichi_image_amd import _native
    v = dict(fx=1000.0, fy=1000.0, cx=32.0, cy=16.0, new_fx=1000.0, new_fy=1000.0, new_cx=32.0, new_cy=16.0)
    v.update(kw)
    return _native.Lens(v["fx"], v["fy"], v["cx"], v["cy"], v["new_fx"], v["new_fy"], v["new_cx"], v["new_cy"],
                        (ctypes.c_double * 8)(0.1, 0.01, 0.001, 0.001, 0.0, 0.0, 0.0, 0.0), n_dist, border)


def test_lens_entry_points_validate_on_the_host():
    from taichi_image_amd import _native
    L = _native.lib()
    assert L.mi_isp_version() >= 1500
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = _lens_arg()
    bad = [_lens_arg(n_dist=3), _lens_arg(n_dist=6), _lens_arg(border=2), _lens_arg(fx=0.0), _lens_arg(fy=-3.0),
           _lens_arg(new_fx=0.0), _lens_arg(new_fy=-1.0), _lens_arg(cx=float("nan")), _lens_arg(new_cy=float("inf")),
           _lens_arg(fx=float("inf")), _lens_arg(cx=1e39)]
    nan_dist = _lens_arg()
    nan_dist.dist[2] = float("nan")
    bad.append(nan_dist)
    big_dist = _lens_arg(n_dist=8)
    big_dist.dist[7] = 1e300
    bad.append(big_dist)
    one = (ctypes.c_void_p * 1)(p)
    for b in bad:
        assert L.mi_isp_undistort(p, p, 32, 64, 32, 64, 1.0, 1.0, 2, 2, b, None) != 0
        assert b"lens" in L.mi_isp_last_error()
        lens_list = (ctypes.c_void_p * 2)(ctypes.addressof(ok), ctypes.addressof(b))
        two = (ctypes.c_void_p * 2)(p, p)
        assert L.mi_isp_undistort_batch(two, two, 2, 32, 64, 32, 64, 1.0, 1.0, 2, 2, lens_list, None) != 0
        assert b"lens" in L.mi_isp_last_error()
    calls = [
        lambda: L.mi_isp_undistort(None, p, 32, 64, 32, 64, 1.0, 1.0, 2, 2, ok, None),
        lambda: L.mi_isp_undistort(p, None, 32, 64, 32, 64, 1.0, 1.0, 2, 2, ok, None),
        lambda: L.mi_isp_undistort(p, p, 32, 64, 32, 64, 1.0, 1.0, 2, 2, None, None),
        lambda: L.mi_isp_undistort(p, p, 0, 64, 32, 64, 1.0, 1.0, 2, 2, ok, None),
        lambda: L.mi_isp_undistort(p, p, 32, -1, 32, 64, 1.0, 1.0, 2, 2, ok, None),
        lambda: L.mi_isp_undistort(p, p, 32, 64, -1, 64, 1.0, 1.0, 2, 2, ok, None),
        lambda: L.mi_isp_undistort(p, p, 32, 64, 32, 64, 1.0, 1.0, 4, 2, ok, None),
        lambda: L.mi_isp_undistort(p, p, 32, 64, 32, 64, 1.0, 1.0, 2, -1, ok, None),
        lambda: L.mi_isp_undistort(p, p, 32, 64, 32, 64, 0.0, 1.0, 2, 2, ok, None),
        lambda: L.mi_isp_undistort(p, p, 32, 64, 32, 64, 1.0, float("nan"), 2, 2, ok, None),
        lambda: L.mi_isp_undistort_batch(None, one, 1, 32, 64, 32, 64, 1.0, 1.0, 2, 2,
                                         (ctypes.c_void_p * 1)(ctypes.addressof(ok)), None),
        lambda: L.mi_isp_undistort_batch(one, one, 1, 32, 64, 32, 64, 1.0, 1.0, 2, 2, (ctypes.c_void_p * 1)(None), None),
        lambda: L.mi_isp_undistort_batch(one, one, 1, 32, 64, 32, 64, 1.0, 1.0, 2, 2, None, None),
        lambda: L.mi_isp_undistort_batch(one, (ctypes.c_void_p * 1)(None), 1, 32, 64, 32, 64, 1.0, 1.0, 2, 2,
                                         (ctypes.c_void_p * 1)(ctypes.addressof(ok)), None),
        lambda: L.mi_isp_undistort_batch(one, one, -1, 32, 64, 32, 64, 1.0, 1.0, 2, 2, None, None),
        lambda: L.mi_isp_remap(p, p, None, 32, 64, 32, 64, 2, 2, 0, None),
        lambda: L.mi_isp_remap(None, p, p, 32, 64, 32, 64, 2, 2, 0, None),
        lambda: L.mi_isp_remap(p, None, p, 32, 64, 32, 64, 2, 2, 0, None),
        lambda: L.mi_isp_remap(p, p, p, 32, 64, 32, 64, 2, 2, 2, None),
        lambda: L.mi_isp_remap(p, p, p, 32, 64, 32, 64, 7, 2, 0, None),
        lambda: L.mi_isp_remap(p, p, p, 0, 64, 32, 64, 2, 2, 0, None),
        lambda: L.mi_isp_remap(p, p, p.value + 4, 32, 64, 32, 64, 2, 2, 0, None),             # table not 8-byte aligned
    ]
    for i, call in enumerate(calls):
        assert call() != 0, i
        assert b"lens" in L.mi_isp_last_error(), (i, L.mi_isp_last_error())
    # nothing to do (no launch, no device): no frames, or an empty output
    assert L.mi_isp_undistort_batch(None, None, 0, 32, 64, 32, 64, 1.0, 1.0, 2, 2, None, None) == 0
    assert L.mi_isp_undistort(p, p, 32, 64, 0, 64, 1.0, 1.0, 2, 2, ok, None) == 0
    assert L.mi_isp_remap(p, p, p, 32, 64, 32, 0, 2, 2, 1, None) == 0


# ---- the scan CLI ---------------------------------------------------------------------------------------------------------
def test_scan_lens_distortion_validated_before_any_frame(tmp_path, monkeypatch):
    from taichi_image_amd.scripts import tonemap_scan as ts
    for cam in ("cam0", "cam1"):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        (tmp_path / "scan" / cam / "f0.raw").write_bytes(b"\0" * 12)

    def no_frames(*a, **k):
        raise AssertionError("a frame was read before the lens files were checked")

    monkeypatch.setattr(ts.ScanIndex, "groups", no_frames)
    ld = tmp_path / "ld"
    ld.mkdir()
    base = ["--scan", str(tmp_path / "scan"), "--width", "8", "--lens-distortion", str(ld), "--device", "cpu"]
    skew = K4K.copy(); skew[0, 1] = 1.0
    cases = [("cam0.npz", dict(K=K4K)),                                     # no dist
             ("cam0.npz", dict(dist=np.zeros(4))),                          # no K
             ("cam0.npz", dict(K=K4K, dist=np.zeros(4), extra=np.zeros(1))),
             ("cam0.npz", dict(K=K4K, dist=np.zeros(6))),
             ("cam0.npz", dict(K=skew, dist=np.zeros(4))),
             ("cam0.npz", dict(K=K4K, dist=np.array([0, np.nan, 0, 0]))),
             ("cam0.npz", dict(K=K4K, dist=np.zeros(4), new_K=-K4K)),
             ("other.npz", dict(K=K4K, dist=np.zeros(4)))]
    for name, arrays in cases:
        for f in ld.iterdir():
            f.unlink()
        np.savez(ld / name, **arrays)
        with pytest.raises(ValueError):
            ts.main(base)
    for f in ld.iterdir():
        f.unlink()
    (ld / "cam0.npz").write_bytes(b"not a zip archive")
    with pytest.raises(ValueError):
        ts.main(base)
    (ld / "cam0.npz").unlink()
    with pytest.raises(FileNotFoundError):
        ts.main(["--scan", str(tmp_path / "scan"), "--lens-distortion", str(tmp_path / "missing"), "--device", "cpu"])
    np.savez(ld / "cam1.npz", K=K4K, dist=np.array([0.1, 0.0, 0.0, 0.0, 0.01]), new_K=K4K)
    calib = ts.load_lens_distortion(ld, ts.ScanIndex.of_scan(tmp_path / "scan").cameras)
    assert list(calib) == ["cam1"] and calib["cam1"]["dist"].tolist() == [0.1, 0.0, 0.0, 0.0, 0.01]
