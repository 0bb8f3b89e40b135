"""Lens distortion correction on the GPU (interpolate.undistort / remap, undistort= of the raw loaders), bit for bit
against the contract of DESIGN.md 3 ("Lens distortion").

Expected values: the oracle's full-resolution loads (O.isp_load_packed12 / 16, O.load_16u / 16f / 32f + O.bayer_to_rgb,
and with levels, shading and defects the CFA of tests/test_gpu_defects.py), then the contract restated in NumPy f32
(tests/test_lens_cpu.py: contract_map, contract_remap); O.metering_images and O.reinhard_isp for the tonemap.  The ramp
test pins the geometry to OpenCV's float64 model instead, independently of the contract's own arithmetic.
"""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_defects import cfa_x, defect_sites
from tests.test_gpu_shading import PER_SITE, make_grid, packed16
from tests.test_lens_cpu import contract_map, contract_remap, opencv_map
from tests.util import assert_close, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
DTYPES = ["u8", "u16", "f16", "f32"]
f32 = np.float32
CCM = O.isp_color_matrix(True, O.DEFAULT_WB, O.DEFAULT_CC)
# OpenCV order; p1 != p2 in sign and size so that a swap shows
DISTS = {4: (-0.32, 0.11, 0.004, -0.0025),
         5: (-0.27, 0.08, -0.0031, 0.0045, -0.02),
         8: (-0.36, 0.19, 0.0035, -0.0021, -0.05, 0.03, 0.012, -0.005)}


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def camera(H, W, k=0):
    return np.array([[0.62 * W + k, 0.0, W / 2 - 0.37 + k], [0.0, 0.6 * W + 1.5 * k, H / 2 + 0.21 - k], [0.0, 0.0, 1.0]])


def wide(K):
    """An output camera with a shorter focal length: the corners sample outside the source (the border rule)."""
    return K * np.array([[0.8], [0.82], [1.0]])


def rand_img(rng, H, W, dt):
    if dt == "u8":
        return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    if dt == "u16":
        return rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    return rng.random((H, W, 3), dtype=np.float32).astype(O.NP_DTYPE[dt])


def out_geometry(H, W, resize_width=0, scale=None):
    """(Hd, Wd, s) of the loaders' resize geometry."""
    sz = O.isp_output_size(H, W, resize_width, scale)
    if sz is None:
        return H, W, 1.0
    (wd, hd), s = sz
    return hd, wd, s


def ref_lens(full, lens, Hd, Wd, s):
    """The contract on a full-resolution oracle image."""
    if lens.is_table:
        return contract_remap(full, lens.table, lens.border)
    m = contract_map(lens.K, lens.dist, Hd, Wd, (s, s), lens.new_K)
    return contract_remap(full, m, lens.border)


# ---- interpolate.undistort / remap ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("din", DTYPES)
@pytest.mark.parametrize("dout", DTYPES)
def test_undistort_every_dtype_pair(ti, rng, dev, din, dout):
    H, W = 198, 250
    src = rand_img(rng, H, W, din)
    t = torch.from_numpy(src).to(dev)
    for n, dist in DISTS.items():
        for border in ("constant", "replicate"):
            K = camera(H, W, n)
            for nK, size, scale in ((None, None, None), (wide(K), (131, 97), None), (wide(K), None, (0.61, 0.55))):
                lens = ti.LensDistortion(K, dist, (H, W), new_K=nK, border=border)
                got = ti.interpolate.undistort(t, lens, size=size, scale=scale, dtype=dout).cpu().numpy()
                if size is not None:
                    Wd, Hd = size
                    s = (Hd / H, Wd / W)
                elif scale is not None:
                    s = scale
                    Hd, Wd = round(H * s[0]), round(W * s[1])
                else:
                    Hd, Wd, s = H, W, (1.0, 1.0)
                ref = contract_remap(src, contract_map(K, dist, Hd, Wd, s, nK), border, dout)
                assert_exact(got, ref, f"{din}->{dout} n={n} {border} size={size} scale={scale}")
    # numpy in, numpy out (the container rule of resize_bilinear)
    lens = ti.LensDistortion(camera(H, W), DISTS[5], (H, W))
    got = ti.interpolate.undistort(src, lens, dtype=dout)
    assert isinstance(got, np.ndarray)
    assert_exact(got, contract_remap(src, contract_map(camera(H, W), DISTS[5], H, W), "constant", dout), "numpy")


@pytest.mark.parametrize("din,dout", [("f16", "f16"), ("f32", "u8"), ("u16", "f32")])
def test_undistort_4k(ti, rng, dev, din, dout):
    H, W = 3072, 4096
    src = rand_img(rng, H, W, din)
    K = camera(H, W)
    for n in (5, 8):
        lens = ti.LensDistortion(K, DISTS[n], (H, W), new_K=wide(K), border="constant" if n == 5 else "replicate")
        got = ti.interpolate.undistort(torch.from_numpy(src).to(dev), lens, dtype=dout).cpu().numpy()
        ref = contract_remap(src, contract_map(K, DISTS[n], H, W, (1, 1), wide(K)), lens.border, dout)
        assert_exact(got, ref, f"n={n}")


@pytest.mark.parametrize("din", DTYPES)
def test_remap_table(ti, rng, dev, din):
    """Random coordinates inside and around the frame, the exact edges, NaN and infinities."""
    H, W = 61, 83
    src = rand_img(rng, H, W, din)
    Hd, Wd = 37, 45
    table = np.stack([rng.uniform(-3, W + 2, (Hd, Wd)), rng.uniform(-3, H + 2, (Hd, Wd))], -1).astype(f32)
    table[0, :6] = [(W - 1, H - 1), (0, 0), (W - 1, 0), (0, H - 1), (np.nan, 3), (np.inf, -np.inf)]
    table[1, :4] = [(W - 1, 5.5), (7.25, H - 1), (np.nextafter(f32(W - 1), f32(W)), 2), (-0.0, 3)]
    for border in ("constant", "replicate"):
        for dout in DTYPES:
            got = ti.interpolate.remap(torch.from_numpy(src).to(dev), table, dtype=dout, border=border).cpu().numpy()
            assert_exact(got, contract_remap(src, table, border, dout), f"{din}->{dout} {border}")


@pytest.mark.parametrize("dt", DTYPES)
def test_identity_table_gives_the_input_bits(ti, rng, dev, dt):
    H, W = 47, 66
    src = rand_img(rng, H, W, dt)
    c, r = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    for border in ("constant", "replicate"):
        got = ti.interpolate.remap(torch.from_numpy(src).to(dev), np.stack([c, r], -1), border=border).cpu().numpy()
        assert_exact(got, src, f"{dt} {border}")


def test_edge_taps_stay_in_the_frame(ti, dev):
    """A sample on the last column (row) has fc = 0 (fr = 0) and its +1 tap clamped to the frame: an infinity at column 0
    of the next row (the next word in memory), or in the row after the frame (the frame is a view of a larger buffer),
    does not reach it."""
    H, W = 9, 16
    big = np.full((H + 2, W, 3), 0.25, np.float32)
    big[:, 0] = np.inf
    big[H:] = np.inf
    table = np.array([[(W - 1, r) for r in range(H - 1)] + [(c, H - 1) for c in range(1, W - 1)]], f32)
    for dt in ("f32", "f16"):
        b = torch.from_numpy(big.astype(O.NP_DTYPE[dt])).to(dev)
        frame = b[:H]                                                      # (a contiguous view: row H follows it)
        s = big[:H].astype(O.NP_DTYPE[dt])
        for border in ("constant", "replicate"):
            got = ti.interpolate.remap(frame, table, border=border).cpu().numpy()
            assert_exact(got, contract_remap(s, table, border), f"{dt} {border}")
            assert np.all(got == s[0, W - 1]), dt


def test_ramp_returns_the_opencv_source_coordinates(ti, dev):
    """R = column, G = row (f32): the undistorted ramp holds the float64 source coordinates of OpenCV's model within
    1e-3 px wherever they fall inside the frame."""
    H, W = 480, 640
    c, r = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    ramp = np.stack([c, r, np.zeros_like(c)], -1)
    for n, dist in DISTS.items():
        K = camera(H, W, n)
        for nK in (None, wide(K)):
            lens = ti.LensDistortion(K, dist, (H, W), new_K=nK)
            got = ti.interpolate.undistort(torch.from_numpy(ramp).to(dev), lens).cpu().numpy().astype(np.float64)
            ref = opencv_map(K, dist, H, W, new_K=nK)
            inside = (ref[..., 0] > 1e-3) & (ref[..., 0] < W - 1 - 1e-3) & (ref[..., 1] > 1e-3) & (ref[..., 1] < H - 1 - 1e-3)
            assert inside.mean() > 0.5
            err = np.abs(got[..., :2] - ref)[inside]
            assert err.max() <= 1e-3, f"n={n}: {err.max():.3e} px"


def test_undistort_arguments(ti, rng, dev):
    H, W = 20, 30
    t = torch.from_numpy(rand_img(rng, H, W, "f16")).to(dev)
    lens = ti.LensDistortion(camera(H, W), DISTS[4], (H, W))
    with pytest.raises(ValueError):
        ti.interpolate.undistort(t[:, :28].contiguous(), lens)              # another frame
    with pytest.raises(ValueError):
        ti.interpolate.undistort(t, "lens")
    with pytest.raises(ValueError):
        ti.interpolate.undistort(t, lens, scale=0.0)
    table = ti.LensDistortion.from_map(np.zeros((5, 6, 2), f32), (H, W))
    assert tuple(ti.interpolate.undistort(t, table).shape) == (5, 6, 3)
    with pytest.raises(ValueError):
        ti.interpolate.undistort(t, table, size=(7, 5))
    with pytest.raises(ValueError):
        ti.interpolate.undistort(t, table, scale=0.5)


# ---- the raw loaders -------------------------------------------------------------------------------------------------------
def _raw(rng, kind, H, W, pattern):
    if kind == "p16":
        return packed16(rng, H, W)
    return natural_packed12(rng, H, W, pattern, ids_format=kind == "ids")


def _load(isp, kind, t, **kw):
    if kind == "p16":
        return isp.load_packed16(t, **kw)
    return isp.load_packed12(t, ids_format=kind == "ids", **kw)


def _full(raw, kind, work, pattern, ccm=None):
    if kind == "p16":
        return O.isp_load_packed16(raw, work, pattern, correct_colors=ccm)
    return O.isp_load_packed12(raw, work, pattern, ids_format=kind == "ids", correct_colors=ccm)


GEOMETRIES = [dict(), dict(resize_width=96), dict(scale=0.7)]


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("pattern", [O.RGGB, O.GRBG, O.GBRG, O.BGGR])
@pytest.mark.parametrize("kind", ["p12", "ids", "p16"])
def test_packed_loaders_bit_exact(ti, rng, dev, cam, work, pattern, kind):
    for (H, W), n in (((64, 256), 5), ((34, 130), 8)):
        raw = _raw(rng, kind, H, W, pattern)
        t = torch.from_numpy(raw).to(dev)
        K = camera(H, W, pattern)
        for geo in GEOMETRIES:
            hd, wd, s = out_geometry(H, W, geo.get("resize_width", 0), geo.get("scale"))
            for cc in (False, True):
                isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=cc, **geo)
                full = _full(raw, kind, work, pattern, CCM if cc else None)
                for lens in (ti.LensDistortion(K, DISTS[n], (H, W), new_K=wide(K), border="replicate"),
                             ti.LensDistortion.from_map(contract_map(K, DISTS[4], hd, wd, (s, s)) + f32(0.37), (H, W))):
                    got = _load(isp, kind, t, undistort=lens)
                    what = f"{cam} {kind} p{pattern} {H}x{W} {geo} ccm={cc} table={lens.is_table}"
                    assert_exact(got.cpu().numpy(), ref_lens(full, lens, hd, wd, s), what)
                    assert getattr(got, "_mi_metering_sub", None) is None, "an untagged image"


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_convert_loaders_bit_exact(ti, rng, dev, cam, work, geo):
    H, W = 34, 130
    u16 = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    u16f = rng.integers(0, 3000, (H, W), dtype=np.uint16)
    fl = rng.random((H, W), dtype=np.float32)
    hd, wd, s = out_geometry(H, W, geo.get("resize_width", 0), geo.get("scale"))
    lens = ti.LensDistortion(camera(H, W), DISTS[8], (H, W), new_K=wide(camera(H, W)))
    for pattern in (O.RGGB, O.BGGR):
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, **geo)
        for fn, src, oracle in ((isp.load_16u, u16, O.load_16u), (isp.load_16f, u16f, O.load_16f),
                                (isp.load_32f, fl, O.load_32f)):
            got = fn(torch.from_numpy(src).to(dev), undistort=lens).cpu().numpy()
            full = O.bayer_to_rgb(oracle(src, work), pattern)
            assert_exact(got, ref_lens(full, lens, hd, wd, s), f"{cam} {fn.__name__} p{pattern} {geo}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "p16"])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_with_levels_shading_and_defects(ti, rng, dev, cam, work, kind, geo):
    H, W = 64, 256
    bits = 16 if kind == "p16" else 12
    white = 3900 if bits == 12 else 60000
    grid = make_grid(rng, 17, 13, 4)
    raw = _raw(rng, kind, H, W, O.GBRG)
    t = torch.from_numpy(raw).to(dev)
    dm = ti.DefectMap(defect_sites(H, W), (H, W))
    hd, wd, s = out_geometry(H, W, geo.get("resize_width", 0), geo.get("scale"))
    lens = ti.LensDistortion(camera(H, W), DISTS[5], (H, W))
    isp = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=PER_SITE, white_level=white, lens_shading=grid,
                           correct_colors=True, **geo)
    xw = cfa_x(raw, bits, work, grid, PER_SITE, white)
    for defects in (None, dm):
        y = xw if defects is None else correct_cfa(xw, dm.mask(), work)
        full = O.bayer_to_rgb(y, O.GBRG, correct_colors=CCM)
        got = _load(isp, kind, t, defects=defects, undistort=lens)
        assert_exact(got.cpu().numpy(), ref_lens(full, lens, hd, wd, s), f"{cam} {kind} {geo} defects={defects}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("geo", GEOMETRIES[:2])
def test_batch_lens_per_camera(ti, rng, dev, cam, work, geo):
    """Six cameras: three analytic lenses (both borders), a table, and two without a lens (one with a defect map): each
    frame as its own call; the frames without a lens keep the bits and the metering tag of the call without lenses."""
    H, W = 64, 256
    hd, wd, s = out_geometry(H, W, geo.get("resize_width", 0))
    raws = [natural_packed12(rng, H, W, O.GRBG) for _ in range(6)]
    ts = [torch.from_numpy(r).to(dev) for r in raws]
    lenses = [ti.LensDistortion(camera(H, W, k), DISTS[(4, 5, 8)[k % 3]], (H, W), border=("constant", "replicate")[k % 2])
              for k in range(3)]
    lenses += [ti.LensDistortion.from_map(contract_map(camera(H, W, 3), DISTS[4], hd, wd, (s, s)), (H, W)), None, None]
    dm = ti.DefectMap(defect_sites(H, W), (H, W))
    maps = [None, dm, None, None, None, dm]
    isp = getattr(ti, cam)(ti.BayerPattern.GRBG, device=dev, **geo)
    got = isp.load_packed12_batch(ts, defects=maps, undistort=lenses)
    plain = isp.load_packed12_batch(ts[4:], defects=maps[4:])
    for k in range(6):
        xw = cfa_x(raws[k], 12, work)
        y = xw if maps[k] is None else correct_cfa(xw, dm.mask(), work)
        full = O.bayer_to_rgb(y, O.GRBG)
        if lenses[k] is None:
            sz = O.isp_output_size(H, W, geo.get("resize_width", 0), None)
            ref = full if sz is None else O.resize_bilinear(full, sz[0], sz[1])
            assert torch.equal(got[k], plain[k - 4]), k
            assert (getattr(got[k], "_mi_metering_sub", None) is None) == (getattr(plain[k - 4], "_mi_metering_sub", None) is None)
        else:
            ref = ref_lens(full, lenses[k], hd, wd, s)
        assert_exact(got[k].cpu().numpy(), ref, f"{cam} {geo} camera {k}")
    with pytest.raises(ValueError):
        isp.load_packed12_batch(ts, undistort=lenses[:5])
    with pytest.raises(ValueError):
        isp.load_packed12_batch(ts, undistort=lenses[0])
    bad_table = ti.LensDistortion.from_map(np.zeros((hd + 1, wd, 2), f32), (H, W))
    with pytest.raises(ValueError):
        isp.load_packed12_batch(ts[:1], undistort=[bad_table])
    with pytest.raises(ValueError):
        isp.load_packed12(ts[0], undistort=bad_table)
    with pytest.raises(ValueError):
        isp.load_packed12(ts[0], undistort=ti.LensDistortion(camera(H, W), DISTS[4], (H, W + 2)))


@pytest.mark.parametrize("cam,work", CAMS)
def test_metering_and_tonemap(ti, rng, dev, cam, work):
    H, W = 80, 128
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, resize_width=64, device=dev)
    hd, wd, s = out_geometry(H, W, 64)
    lenses = [ti.LensDistortion(camera(H, W, k), DISTS[(4, 5, 8)[k]], (H, W)) for k in range(3)]
    st = O.IspState(0.3)
    for step in range(3):
        packs = [natural_packed12(rng, H, W, dark=0.05 * step) for _ in range(3)]
        imgs = isp.load_packed12_batch([torch.from_numpy(p).to(dev) for p in packs], undistort=lenses)
        refs = [ref_lens(O.isp_load_packed12(p, work), ln, hd, wd, s) for p, ln in zip(packs, lenses)]
        for im, r in zip(imgs, refs):
            assert_exact(im.cpu().numpy(), r, f"image step {step}")
        outs = isp.tonemap_reinhard(imgs, gamma=0.6)
        m = st.update_metering(refs)
        assert_close(isp.metrics.cpu().numpy(), m, f"metrics step {step}", rel=2e-5)
        for k, (o, r) in enumerate(zip(outs, refs)):
            assert_close(o.cpu().numpy(), O.reinhard_isp(r, m, gamma=0.6)[0], f"u8 step {step} img {k}")


def test_process_packed12_takes_the_two_calls(ti, rng, dev, monkeypatch):
    from taichi_image_amd import _native, synthetic
    L = _native.lib()
    frames = [torch.from_numpy(synthetic.synthetic_packed12(k, 3072, 4096)).to(dev) for k in range(2)]
    K = camera(3072, 4096)
    lenses = [ti.LensDistortion(K, DISTS[5], (3072, 4096)), None]
    a = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev)
    b = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev)
    calls = []
    group = L.mi_isp_camera_group_reinhard
    monkeypatch.setattr(L, "mi_isp_camera_group_reinhard", lambda *args: calls.append(1) or group(*args))
    for step in range(2):
        outs, imgs = a.process_packed12(frames, gamma=0.6, keep_images=True, undistort=lenses)
        imgs_b = b.load_packed12_batch(frames, undistort=lenses)
        outs_b = b.tonemap_reinhard(imgs_b, gamma=0.6)
        assert torch.equal(a.metrics, b.metrics), f"metering state, step {step}"
        for k in range(2):
            assert torch.equal(outs[k], outs_b[k]), f"u8 output {k}, step {step}"
            assert torch.equal(imgs[k].view(torch.int16), imgs_b[k].view(torch.int16)), f"image {k}, step {step}"
    assert not calls, "process_packed12 with a lens took the camera-group kernel"
    with pytest.raises(ValueError):
        a.process_packed12(frames, undistort=lenses[:1])


def test_graph_capture_with_a_cached_table(ti, rng, dev):
    """A table lens used once is cached on the device: a captured loader call makes no copy and replays the same bits."""
    H, W = 64, 256
    raw = natural_packed12(rng, H, W)
    t = torch.from_numpy(raw).to(dev)
    isp = ti.Camera16(ti.BayerPattern.RGGB, resize_width=128, device=dev)
    hd, wd, s = out_geometry(H, W, 128)
    lens = ti.LensDistortion.from_map(contract_map(camera(H, W), DISTS[8], hd, wd, (s, s)), (H, W), border="replicate")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        first = isp.load_packed12(t, undistort=lens)                      # (uploads the table)
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = isp.load_packed12(t, undistort=lens)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), first.view(torch.int16))
    assert_exact(out.cpu().numpy(), ref_lens(O.isp_load_packed12(raw, "f16"), lens, hd, wd, s), "replay")


@pytest.mark.parametrize("cam,work", CAMS)
def test_undistort_none_is_the_call_without_it(ti, rng, dev, cam, work):
    H, W = 64, 256
    raws = [natural_packed12(rng, H, W) for _ in range(2)]
    ts = [torch.from_numpy(r).to(dev) for r in raws]
    p16 = torch.from_numpy(packed16(rng, H, W)).to(dev)
    u16 = torch.from_numpy(rng.integers(0, 65536, (H, W), dtype=np.uint16)).to(dev)
    for geo in GEOMETRIES:
        isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, **geo)
        pairs = [(isp.load_packed12(ts[0]), isp.load_packed12(ts[0], undistort=None)),
                 (isp.load_packed16(p16), isp.load_packed16(p16, undistort=None)),
                 (isp.load_16u(u16), isp.load_16u(u16, undistort=None))]
        pairs += list(zip(isp.load_packed12_batch(ts), isp.load_packed12_batch(ts, undistort=[None, None])))
        pairs += list(zip(isp.load_packed12_batch(ts), isp.load_packed12_batch(ts, undistort=None)))
        for k, (a, b) in enumerate(pairs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (geo, k)
            ta, tb = getattr(a, "_mi_metering_sub", None), getattr(b, "_mi_metering_sub", None)
            assert (ta is None) == (tb is None), (geo, k)
            if ta is not None:
                assert torch.equal(ta[0].view(torch.uint8), tb[0].view(torch.uint8)), (geo, k)
