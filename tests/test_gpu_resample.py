"""The antialiased resize (interpolate.resample, Camera16/32 resample=, mi_isp_resample_batch) on the GPU against
tests/resample_ref.py fed with the library's own tables, bit for bit.

The kernel's tile is 64 x 32 outputs (OW x OH) and it walks the source rows four at a time.  CASES are one tile, one tile
+ 1 and two tiles + 1 each way, D = 1, a source smaller than the taps, scale 1 (the identity), scale 2, a per-axis pair, a
square image whose axes differ in scale only (exchanged tables would still fit it),
scale 1/4 (the widest tables all three filters take) and, for area and triangle, scale 1/8, where a tile's columns span
more than the 512 source pixels of the LDS segment and the taps are read from memory instead.  The coverage condition
(first and last tap non-zero somewhere, start at both ends) is asserted on the reference alone."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import resample_ref as R
from tests.util import _count_calls, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

S3 = 240 / 512
# name: (Hs, Ws, Hd, Wd, row scale, col scale)
CASES = {
    "tile": (69, 137, 32, 64, S3, S3),
    "tile+1": (71, 139, 33, 65, S3, S3),
    "tiles+1": (139, 276, 65, 129, S3, S3),
    "d1": (5, 6, 1, 1, 0.25, 0.25),
    "small": (3, 5, 2, 2, 0.4, 0.4),
    "one": (37, 70, 37, 70, 1.0, 1.0),
    "two": (20, 33, 40, 66, 2.0, 2.0),
    "pair": (139, 172, 65, 129, 0.469, 0.75),
    "square": (100, 100, 47, 47, 0.469, 0.5),
    "quarter": (140, 264, 35, 66, 0.25, 0.25),
    "eighth": (264, 520, 33, 65, 0.125, 0.125),
}
FILTERS = R.FILTERS
PAIRS = [("f16", "f16"), ("f16", "f32"), ("f32", "f16"), ("f32", "f32")]
NP = {"f16": np.float16, "f32": np.float32}
INF_AT = (5, 7, 1)                       # in "two": column 7 is the zero-weight second tap of the even outputs 12 and 14


def cases_of(filt):
    return [c for c in CASES if not (c == "eighth" and filt == "lanczos3")]


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def tables(case, filt):
    """The library's own tables of a case: (rows, cols), each (T, start, weight)."""
    from taichi_image_amd import resample as rs
    Hs, Ws, Hd, Wd, s0, s1 = CASES[case]
    return rs.table(filt, Hs, Hd, s0), rs.table(filt, Ws, Wd, s1)


def source(case, work, k=0):
    """Image k of a case: random values in [-1, 3); the f16 source of "two" holds an inf."""
    Hs, Ws = CASES[case][:2]
    rng = np.random.default_rng(list(CASES).index(case) * 16 + k)
    x = (rng.random((Hs, Ws, 3), dtype=np.float32) * 4 - 1).astype(NP[work])
    if case == "two" and work == "f16" and k == 0:
        x[INF_AT] = np.inf
    return x


_refs: dict = {}


def reference(case, filt, work, k=0):
    """The f32 result of the restatement on the library's tables, computed once and shared; never written."""
    key = (case, filt, work, k)
    if key not in _refs:
        rows, cols = tables(case, filt)
        _refs[key] = R.resample(source(case, work, k), rows, cols, np.float32)
        _refs[key].setflags(write=False)
    return _refs[key]


def cast(ref32, out):
    with np.errstate(over="ignore", invalid="ignore"):
        return ref32.astype(NP[out])


def assert_same(got, want, what):
    """Bit for bit, a nan for a nan."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: the nans differ"
    assert_exact(np.where(nan, 0, got), np.where(nan, 0, want), what)


@pytest.mark.parametrize("filt", FILTERS)
def test_the_cases_cover_the_tables(filt):
    """On the reference alone: over the case list the first and the last tap of a row carry a non-zero weight somewhere,
    start hits both 0 and S - T, and the inf of "two" sits under a zero weight."""
    first = last = lo = hi = False
    for case in cases_of(filt):
        Hs, Ws, Hd, Wd, s0, s1 = CASES[case]
        for S, D, s in ((Hs, Hd, s0), (Ws, Wd, s1)):
            T, start, weight = R.table(filt, S, D, s)
            if T > 1 and D > 1:
                first |= bool((weight[:, 0] != 0).any()) and bool((weight[:, 0] == 0).any())
                last |= bool((weight[:, -1] != 0).any()) and bool((weight[:, -1] == 0).any())
                lo |= bool((start == 0).any())
                hi |= bool((start == S - T).any()) and S - T > 0
    assert first and last and lo and hi
    T, start, weight = R.table(filt, 33, 66, 2.0)
    reach = [(d, INF_AT[1] - start[d]) for d in range(66) if 0 <= INF_AT[1] - start[d] < T]
    assert any(weight[d, j] == 0 for d, j in reach)


@pytest.mark.parametrize("tin,tout", PAIRS)
@pytest.mark.parametrize("filt", FILTERS)
def test_resample_is_the_restatement(ti, dev, filt, tin, tout):
    for case in cases_of(filt):
        Hs, Ws, Hd, Wd, s0, s1 = CASES[case]
        src = source(case, tin)
        got = ti.interpolate.resample(torch.from_numpy(src).to(dev), (Wd, Hd), (s0, s1), filt, dtype=tout)
        want = cast(reference(case, filt, tin), tout)
        assert_same(got.cpu().numpy(), want, f"{filt} {case} {tin}->{tout}")
        if case == "two" and tin == "f16":
            assert np.isnan(want).any(), "the inf must reach a padded tap"
        if case == "one" and tin == tout:
            assert_exact(got.cpu().numpy(), src, f"{filt} scale 1 is the identity")
    # numpy in, numpy out
    out = ti.interpolate.resample(source("tile+1", tin), (65, 33), S3, filt, dtype=tout)
    assert isinstance(out, np.ndarray)
    assert_same(out, cast(reference("tile+1", filt, tin), tout), f"{filt} numpy {tin}->{tout}")


@pytest.mark.parametrize("tin,tout", PAIRS)
@pytest.mark.parametrize("filt", FILTERS)
def test_a_batch_of_three_is_one_launch(ti, dev, monkeypatch, filt, tin, tout):
    from taichi_image_amd import resample as rs
    from taichi_image_amd import types
    n_calls = _count_calls(monkeypatch, "mi_isp_resample_batch")
    for case in ("tiles+1", "pair", "small"):
        Hs, Ws, Hd, Wd, s0, s1 = CASES[case]
        srcs = [torch.from_numpy(source(case, tin, k)).to(dev) for k in range(3)]
        dsts = [torch.full((Hd, Wd, 3), 7.0, dtype=types.as_dtype(tout).torch, device=dev) for _ in range(3)]
        n_calls.clear()
        rs.apply(srcs, dsts, filt, Hs, Ws, Hd, Wd, s0, s1, types.as_dtype(tin).code, types.as_dtype(tout).code, dev)
        assert len(n_calls) == 1
        for k in range(3):
            assert_same(dsts[k].cpu().numpy(), cast(reference(case, filt, tin, k), tout), f"{filt} {case} image {k}")


@pytest.mark.parametrize("tin,tout", [("f16", "f16"), ("f32", "f32")])
def test_tables_whose_starts_do_not_rise(ti, dev, tin, tout):
    """The kernel evaluates any table: random starts within [0, S - T] (no order: the ring cannot hold such a tile's rows
    and the tile is evaluated from memory) and random weights, through the C entry point."""
    import ctypes
    from taichi_image_amd import _native, types
    rng = np.random.default_rng(5)
    Hs, Ws, Hd, Wd, Ty, Tx = 90, 150, 40, 70, 5, 7
    rows = (Ty, rng.integers(0, Hs - Ty + 1, Hd).astype(np.int32), rng.standard_normal((Hd, Ty)).astype(np.float32))
    cols = (Tx, rng.integers(0, Ws - Tx + 1, Wd).astype(np.int32), rng.standard_normal((Wd, Tx)).astype(np.float32))
    rows[1][:2], cols[1][:2] = (0, Hs - Ty), (Ws - Tx, 0)
    src = (rng.random((Hs, Ws, 3), dtype=np.float32) * 4 - 1).astype(NP[tin])
    want = R.resample(src, rows, cols, NP[tout])
    t = torch.from_numpy(src).to(dev)
    out = torch.empty((Hd, Wd, 3), dtype=types.as_dtype(tout).torch, device=dev)
    held = [torch.from_numpy(x).to(dev) for x in (rows[1], rows[2], cols[1], cols[2])]
    ax = [_native.ResampleAxis(Ty, held[0].data_ptr(), held[1].data_ptr()),
          _native.ResampleAxis(Tx, held[2].data_ptr(), held[3].data_ptr())]
    _native.check(_native.lib().mi_isp_resample_batch(
        _native.ptr_array([t]), _native.ptr_array([out]), 1, Hs, Ws, Hd, Wd, types.as_dtype(tin).code,
        types.as_dtype(tout).code, ctypes.byref(ax[0]), ctypes.byref(ax[1]), _native.stream_ptr(dev)))
    assert_same(out.cpu().numpy(), want, f"random tables {tin}")


def test_scale_none_is_the_geometric_scale_and_bilinear_is_resize_bilinear(ti, dev):
    src = source("tiles+1", "f32")
    Hs, Ws = src.shape[:2]
    t = torch.from_numpy(src).to(dev)
    got = ti.interpolate.resample(t, (100, 60), filter="triangle")
    want = ti.interpolate.resample(t, (100, 60), (60 / Hs, 100 / Ws), "triangle")
    assert torch.equal(got, want)
    rows, cols = R.table("triangle", Hs, 60, 60 / Hs), R.table("triangle", Ws, 100, 100 / Ws)
    assert np.abs(got.cpu().numpy() - R.resample(src, rows, cols)).max() < 1e-5
    bil = ti.interpolate.resample(t, (129, 65), S3, "bilinear")
    assert torch.equal(bil, ti.interpolate.resize_bilinear(t, (129, 65), S3))


def test_a_cached_geometry_is_captured_into_a_graph(ti, dev):
    Hs, Ws, Hd, Wd, s0, s1 = CASES["tiles+1"]
    t = torch.from_numpy(source("tiles+1", "f16")).to(dev)
    first = ti.interpolate.resample(t, (Wd, Hd), (s0, s1), "lanczos3")       # (uploads the tables)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ti.interpolate.resample(t, (Wd, Hd), (s0, s1), "lanczos3")
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    assert_same(out.cpu().numpy(), cast(reference("tiles+1", "lanczos3", "f16"), "f16"), "graph replay")


# ---- the ISP ----------------------------------------------------------------------------------------------------------
CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
H, W, RW = 96, 128, 60                   # scale 0.46875: 96 x 128 -> 45 x 60


def resampled(full, filt):
    """A full-resolution work-dtype image through the restatement at the ISP's geometry, on the library's tables."""
    from taichi_image_amd import resample as rs
    h, w = full.shape[:2]
    s = RW / w
    return R.resample(full, rs.table(filt, h, round(h * s), s), rs.table(filt, w, RW, s))


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(11)
    return [natural_packed12(rng, H, W) for _ in range(3)]


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("filt", FILTERS)
def test_loaders(ti, dev, monkeypatch, frames, cam, work, filt):
    """load_packed12, load_packed12_batch (ONE resample launch) and load_16u: the oracle's full-resolution image through
    the restatement; the images carry no metering subsample; tonemap_reinhard follows as on any image."""
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, resize_width=RW, resample=ti.Resample(filt), moving_alpha=1.0)
    assert isp.resample == ti.Resample(filt)
    ts = [torch.from_numpy(f).to(dev) for f in frames]
    want = [resampled(O.isp_load_packed12(f, work), filt) for f in frames]
    img = isp.load_packed12(ts[0])
    assert getattr(img, "_mi_metering_sub", None) is None
    assert_exact(img.cpu().numpy(), want[0], f"{cam} {filt} load_packed12")
    n_rs = _count_calls(monkeypatch, "mi_isp_resample_batch")
    n_bil = _count_calls(monkeypatch, "mi_isp_resize_bilinear")
    imgs = isp.load_packed12_batch(ts)
    assert len(n_rs) == 1 and not n_bil
    for k in range(3):
        assert_exact(imgs[k].cpu().numpy(), want[k], f"{cam} {filt} batch image {k}")
    codes = torch.from_numpy((O.decode12(frames[0], "u16", scaled=False).astype(np.uint16) * 16)).to(dev)
    full = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev).load_16u(codes).cpu().numpy()    # (pinned by its own files)
    assert_exact(isp.load_16u(codes).cpu().numpy(), resampled(full, filt), f"{cam} {filt} load_16u")
    # the tonemap on the resampled images is the tonemap on any image of those bits
    outs = isp.tonemap_reinhard([im.clone() for im in imgs], gamma=0.7)
    other = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, moving_alpha=1.0)
    ref = other.tonemap_reinhard([torch.from_numpy(w).to(dev) for w in want], gamma=0.7)
    for o, r in zip(outs, ref):
        assert torch.equal(o, r)


@pytest.mark.parametrize("cam,work", CAMS)
def test_defect_map_lens_and_directional(ti, dev, monkeypatch, frames, cam, work):
    """Each stage in front of the resize runs at full resolution, as on an ISP without a resize (each pinned by its own
    files), and the restatement resizes its image."""
    Cam = getattr(ti, cam)
    ts = [torch.from_numpy(f).to(dev) for f in frames]
    on = dict(device=dev, resize_width=RW, resample=ti.Resample("area"))
    m = ti.DefectMap([(0, 0), (30, 31), (31, 64), (95, 127), (33, 0)], (H, W))
    K = np.array([[110.0, 0, W / 2 - 3], [0, 112.0, H / 2 + 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, (-0.2, 0.05, 0.001, -0.002), (H, W))
    for what, ctor, call in (
            ("defects", {}, dict(defects=[m, None, m])),
            ("lens", {}, dict(undistort=[lens, None, lens])),
            ("directional", dict(demosaic=ti.Demosaic("directional")), {}),
            ("directional + defects + lens", dict(demosaic=ti.Demosaic("directional")),
             dict(defects=[m, None, None], undistort=[None, lens, None]))):
        isp, plain = Cam(ti.BayerPattern.GRBG, **on, **ctor), Cam(ti.BayerPattern.GRBG, device=dev, **ctor)
        n_rs = _count_calls(monkeypatch, "mi_isp_resample_batch")
        imgs = isp.load_packed12_batch(ts, **call)
        assert len(n_rs) == 1, what
        full = plain.load_packed12_batch(ts, **call)
        for k in range(3):
            assert full[k].shape == (H, W, 3)
            assert_exact(imgs[k].cpu().numpy(), resampled(full[k].cpu().numpy(), "area"), f"{cam} {what} image {k}")
        one = isp.load_packed12(ts[0], **{k: v[0] for k, v in call.items()})
        assert torch.equal(one, imgs[0]), what
    # a table lens has the frame's shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    table = ti.LensDistortion.from_map(np.stack([xs * 0.98 + 1, ys * 0.97 + 1], -1), (H, W), "replicate")
    isp, plain = Cam(ti.BayerPattern.RGGB, **on), Cam(ti.BayerPattern.RGGB, device=dev)
    got = isp.load_packed12(ts[1], undistort=table)
    assert_exact(got.cpu().numpy(), resampled(plain.load_packed12(ts[1], undistort=table).cpu().numpy(), "area"), "table lens")


def test_process_packed12_is_the_two_calls(ti, dev, frames):
    ts = [torch.from_numpy(f).to(dev) for f in frames]
    kw = dict(device=dev, moving_alpha=0.3, correct_colors=True, resize_width=RW, resample=ti.Resample("triangle"))
    a, b = ti.Camera16(ti.BayerPattern.RGGB, **kw), ti.Camera16(ti.BayerPattern.RGGB, **kw)
    for _ in range(2):
        outs = a.process_packed12(ts, gamma=0.8)
        want = b.tonemap_reinhard(b.load_packed12_batch(ts), gamma=0.8)
        for o, w in zip(outs, want):
            assert torch.equal(o, w)
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), "metering")
    kw.pop("resample")
    plain = ti.Camera16(ti.BayerPattern.RGGB, **kw)
    assert not torch.equal(plain.process_packed12(ts, gamma=0.8)[0], outs[0]), "the option must change the image"


@pytest.mark.parametrize("cam,work", CAMS)
def test_option_off_gives_the_bytes_and_the_launches_of_today(ti, dev, monkeypatch, frames, cam, work):
    """resample=None, Resample("bilinear"), set(resample=False) and a filter without a resize: the oracle's bits and, entry
    point by entry point, the calls of an ISP that never had the option."""
    from taichi_image_amd import _native
    Cam = getattr(ti, cam)
    ts = [torch.from_numpy(f).to(dev) for f in frames]
    counts = {n: _count_calls(monkeypatch, n) for n in _native.SIGNATURES if n != "mi_isp_last_error"}

    def run(isp):
        for c in counts.values():
            c.clear()
        imgs = [isp.load_packed12(ts[0])] + isp.load_packed12_batch(ts)
        outs = isp.process_packed12(ts, gamma=0.8)
        return [x.cpu().numpy() for x in imgs + outs], {n: len(c) for n, c in counts.items()}

    base, base_calls = run(Cam(ti.BayerPattern.RGGB, device=dev, resize_width=RW))
    assert_exact(base[0], O.isp_load_packed12(frames[0], work, resize_width=RW), "today's bits")
    assert base_calls["mi_isp_resample_batch"] == 0
    area = Cam(ti.BayerPattern.RGGB, device=dev, resize_width=RW, resample=ti.Resample("area"))
    assert not np.array_equal(run(area)[0][0], base[0]), "the option must change the image"
    turned = Cam(ti.BayerPattern.RGGB, device=dev, resize_width=RW, resample=ti.Resample("area"))
    turned.set(moving_alpha=0.1)
    assert turned.resample is not None
    turned.set(resample=False)
    assert turned.resample is None
    for isp in (Cam(ti.BayerPattern.RGGB, device=dev, resize_width=RW, resample=ti.Resample("bilinear")), turned):
        got, calls = run(isp)
        assert calls == base_calls
        for g, b in zip(got, base):
            assert_exact(g, b, f"{cam} option off")
    # without a resize the option has no effect
    full, full_calls = run(Cam(ti.BayerPattern.RGGB, device=dev))
    got, calls = run(Cam(ti.BayerPattern.RGGB, device=dev, resample=ti.Resample("lanczos3")))
    assert calls == full_calls
    for g, b in zip(got, full):
        assert_exact(g, b, f"{cam} no resize")
