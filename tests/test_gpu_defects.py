"""Defective pixel correction (defects= of the raw loaders) on the GPU, bit for bit against the oracle.

Expected values: the raw codes (O.decode12 / O.decode16 unscaled), levels and shading as tests/test_gpu_shading.py computes
them, the contract of DESIGN.md 3 restated in NumPy (tests/test_defects_cpu.py: correct_cfa), then O.bayer_to_rgb,
O.resize_bilinear and O.metering_images; at 4096 x 3072 the C oracle's demosaic of the corrected CFA.
"""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_shading import PER_SITE, make_grid, packed16, pixel_gains, raw_x
from tests.util import assert_close, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
WORK_CODE = {"f16": 2, "f32": 3}
f32 = np.float32
CCM = O.isp_color_matrix(True, O.DEFAULT_WB, O.DEFAULT_CC)


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def defect_sites(H, W):
    """Interior sites, all four borders and corners, a 2x2 cluster, a same-site cross that forces the diagonal fallback at
    its centre, and a site with all eight same-site neighbours defective (kept)."""
    s = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2 + 1), (H - 1, W // 3), (H // 2 + 1, 0),
         (H // 2, W - 1), (1, 1), (H - 2, W - 2), (1, W - 2), (5, 9), (7, 2 * W // 3)}
    s |= {(10, 20), (10, 21), (11, 20), (11, 21)}
    s |= {(18, 40), (16, 40), (20, 40), (18, 38), (18, 42)}
    s |= {(26, 60)} | {(26 + dr, 60 + dc) for dr in (-2, 0, 2) for dc in (-2, 0, 2)}
    return sorted((r, c) for r, c in s if 0 <= r < H and 0 <= c < W)


def cfa_x(raw, bits, work, grid=None, black=None, white=None, ids_format=False):
    """The work-dtype CFA the loader gives today (levels and shading included)."""
    codes = O.decode12(raw, "u16", ids_format=ids_format) if bits == 12 else O.decode16(raw, "u16")
    x = raw_x(codes, bits, black, white)
    if grid is not None:
        x = x * pixel_gains(grid, *codes.shape)
    return O.cast_out(x, work)


def ref_rgb(xw, mask, work, pattern, ccm=None, resize_width=0, scale=None):
    y = xw if mask is None else correct_cfa(xw, mask, work)
    rgb = O.bayer_to_rgb(y, pattern, correct_colors=ccm)
    sz = O.isp_output_size(rgb.shape[0], rgb.shape[1], resize_width, scale)
    return rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1])


def _raw(rng, kind, H, W, pattern):
    if kind == "p16":
        return packed16(rng, H, W)
    return natural_packed12(rng, H, W, pattern, ids_format=kind == "ids")


def _load(isp, kind, t, **kw):
    if kind == "p16":
        return isp.load_packed16(t, **kw)
    return isp.load_packed12(t, ids_format=kind == "ids", **kw)


SHAPES = [(64, 256), (34, 130)]       # the stream (metered) route for standard packed-12, and the tile route


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("pattern", [O.RGGB, O.GRBG, O.GBRG, O.BGGR])
@pytest.mark.parametrize("kind", ["p12", "ids", "p16"])
def test_packed_loaders_bit_exact(ti, rng, dev, cam, work, pattern, kind):
    from taichi_image_amd import _native
    L = _native.lib()
    bits = 16 if kind == "p16" else 12
    grid = make_grid(rng, 17, 13, 4)
    for H, W in SHAPES:
        m = ti.DefectMap(defect_sites(H, W), (H, W))
        mask = m.mask()
        raw = _raw(rng, kind, H, W, pattern)
        t = torch.from_numpy(raw).to(dev)
        metered = bool(L.mi_isp_load_packed_metered_is_fused(H, W, bits, int(kind == "ids"), WORK_CODE[work], 8))
        assert metered == (kind == "p12" and W % 8 == 0), "the route under test"
        for black, white, g in ((None, None, None), (PER_SITE, 3900 if bits == 12 else 60000, grid)):
            for cc in (False, True):
                isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white,
                                       lens_shading=g, correct_colors=cc)
                xw = cfa_x(raw, bits, work, g, black, white, ids_format=kind == "ids")
                ref = ref_rgb(xw, mask, work, pattern, CCM if cc else None)
                got = _load(isp, kind, t, defects=m)
                what = f"{cam} {kind} p{pattern} {H}x{W} levels={black is not None} ccm={cc}"
                assert_exact(got.cpu().numpy(), ref, what)
                sub = getattr(got, "_mi_metering_sub", None)
                assert (sub is not None) == metered
                if sub is not None:
                    assert_exact(sub[0].cpu().numpy(), ref[::8, ::8], what + " metering subsample")


@pytest.mark.parametrize("cam,work", CAMS)
def test_metering_subsample_strides(ti, rng, dev, cam, work):
    """Stride 8 through the metered loader, stride 3 through update_metering and through the C entry points directly."""
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = 64, 256
    m = ti.DefectMap(defect_sites(H, W) + [(24, 24), (24, 27), (3, 6)], (H, W))
    raw = natural_packed12(rng, H, W, O.GBRG)
    ref = ref_rgb(cfa_x(raw, 12, work), m.mask(), work, O.GBRG)
    t = torch.from_numpy(raw).to(dev)
    for st in (8, 3):
        isp = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, metering_stride=st, moving_alpha=1.0)
        img = isp.load_packed12(t, defects=m)
        assert_exact(img.cpu().numpy(), ref, f"stride {st}")
        isp.update_metering([img])
        assert_close(isp.metrics.cpu().numpy(), O.metering_images([ref], 0.0, np.zeros(9, f32), st), f"metering {st}")
    # the fix-up's own subsample path at stride 3
    rgb = torch.empty((H, W, 3), dtype=getattr(torch, {"f16": "float16", "f32": "float32"}[work]), device=dev)
    sub = torch.full(((H + 2) // 3, (W + 2) // 3, 3), 7.0, dtype=rgb.dtype, device=dev)
    stream = _native.stream_ptr(dev)
    _native.check(L.mi_isp_load_packed_metered(t.data_ptr(), rgb.data_ptr(), H, W, 12, 0, O.GBRG, None, WORK_CODE[work],
                                               H, W, 0.0, sub.data_ptr(), 3, stream))
    lst, n = m._outputs(dev, H, W, 0.0)
    _native.check(L.mi_isp_defects_fix_packed(t.data_ptr(), rgb.data_ptr(), H, W, 12, 0, O.GBRG, None, WORK_CODE[work],
                                              H, W, 0.0, sub.data_ptr(), 3, None, None, m._arg(dev), lst.data_ptr(), n,
                                              stream))
    assert_exact(rgb.cpu().numpy(), ref, "C entry point")
    assert_exact(sub.cpu().numpy(), ref[::3, ::3], "C entry point, stride-3 subsample")


def _resize_sites(H, W, scale, n=48):
    """Sites at every row and column phase of the resize grid (the fractional part of i / scale) plus the frame's edges."""
    s = {(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)}
    for k in range(n):
        r = int(f32(2 * k + 1) / f32(scale)) + (k % 3)
        c = int(f32(3 * k + 2) / f32(scale)) + (k % 4)
        s.add((min(r, H - 1), min(c, W - 1)))
    return sorted(s)


@pytest.mark.parametrize("cam,work", CAMS)
def test_resize_scale_sweep(ti, rng, dev, cam, work):
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = 96, 256
    raw = natural_packed12(rng, H, W, O.GRBG)
    t = torch.from_numpy(raw).to(dev)
    grid = make_grid(rng, 9, 9, 4)
    for rw in (128, 64, 200, 96, 120, 512):
        scale = rw / W
        m = ti.DefectMap(_resize_sites(H, W, scale), (H, W))
        for black, g in ((None, None), (PER_SITE, grid)):
            isp = getattr(ti, cam)(ti.BayerPattern.GRBG, resize_width=rw, device=dev, black_level=black, lens_shading=g)
            ref = ref_rgb(cfa_x(raw, 12, work, g, black), m.mask(), work, O.GRBG, resize_width=rw)
            got = isp.load_packed12(t, defects=m).cpu().numpy()
            assert_exact(got, ref, f"{cam} resize_width={rw} (fused {bool(L.mi_isp_load_packed_scale_supported(scale))})")


@pytest.mark.parametrize("cam,work", CAMS)
def test_resize_4k_to_1920(ti, rng, dev, cam, work):
    from oracle import c_oracle
    from taichi_image_amd import _native, synthetic
    H, W = 3072, 4096
    assert _native.lib().mi_isp_load_packed_scale_supported(1920 / 4096), "the fused resize route"
    raw = synthetic.synthetic_packed12(5, H, W)
    sites = _resize_sites(H, W, 1920 / 4096, n=400) + defect_sites(H, W)
    sites += [(int(r), int(c)) for r, c in rng.integers(0, [H, W], (2000, 2))]
    m = ti.DefectMap(sites, (H, W))
    xw = cfa_x(raw, 12, work)
    y = correct_cfa(xw, m.mask(), work)
    rgb = c_oracle.demosaic(y.astype(f32), O.RGGB, round_f16=work == "f16")
    rgb = rgb.astype(np.float16) if work == "f16" else rgb
    ref = O.resize_bilinear(rgb, (1920, 1440), 1920 / 4096)
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, resize_width=1920, device=dev)
    got = isp.load_packed12_batch([torch.from_numpy(raw).to(dev)] * 2, defects=[m, None])
    assert_exact(got[0].cpu().numpy(), ref, f"{cam} 4096x3072 -> 1920 with defects")
    assert_exact(got[1].cpu().numpy(), O.resize_bilinear(c_oracle.demosaic(xw.astype(f32), O.RGGB,
                                                                           round_f16=work == "f16").astype(xw.dtype),
                                                         (1920, 1440), 1920 / 4096), f"{cam} 4096x3072 -> 1920 no map")


@pytest.mark.parametrize("cam,work", CAMS)
def test_batch_six_cameras(ti, rng, dev, cam, work):
    for (H, W), rw in (((64, 256), 0), ((34, 130), 0), ((96, 256), 128)):
        frames = [natural_packed12(rng, H, W, O.BGGR, dark=0.02 * k) for k in range(6)]
        maps = []
        for k in range(6):
            extra = [(int(r), int(c)) for r, c in rng.integers(0, [H, W], (3 + 5 * k, 2))]
            maps.append(None if k == 2 else ti.DefectMap(defect_sites(H, W)[k:] + extra, (H, W)))
        isp = getattr(ti, cam)(ti.BayerPattern.BGGR, resize_width=rw, device=dev, black_level=PER_SITE, white_level=4000)
        ts = [torch.from_numpy(f).to(dev) for f in frames]
        got = isp.load_packed12_batch(ts, defects=maps)
        for k, (g, f, m) in enumerate(zip(got, frames, maps)):
            ref = ref_rgb(cfa_x(f, 12, work, None, PER_SITE, 4000), None if m is None else m.mask(), work, O.BGGR,
                          resize_width=rw)
            assert_exact(g.cpu().numpy(), ref, f"{cam} batch {H}x{W} camera {k}")
            single = isp.load_packed12(ts[k], defects=m)
            assert_exact(single.cpu().numpy(), ref, f"{cam} single {H}x{W} camera {k}")
            sub = getattr(g, "_mi_metering_sub", None)
            if sub is not None:
                assert_exact(sub[0].cpu().numpy(), ref[::8, ::8], f"{cam} batch subsample {k}")
    with pytest.raises(ValueError):
        isp.load_packed12_batch(ts, defects=maps[:5])
    with pytest.raises(ValueError):
        isp.load_packed12_batch(ts, defects=[ti.DefectMap([[0, 0]], (H, W + 2))] + [None] * 5)
    with pytest.raises(ValueError):
        isp.load_packed12(ts[0], defects=ti.DefectMap([[0, 0]], (H + 2, W)))


@pytest.mark.parametrize("cam,work", CAMS)
def test_convert_loaders(ti, rng, dev, cam, work):
    H, W = 34, 130
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    u16 = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    fl = rng.random((H, W), dtype=np.float32)
    grid = make_grid(rng, 9, 9, 4)
    for g in (None, grid):
        gain = np.ones((H, W), f32) if g is None else pixel_gains(g, H, W)
        isp = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, lens_shading=g, correct_colors=True)
        cases = [(isp.load_16u, u16, u16.astype(f32) / f32(65535.0)), (isp.load_16f, u16 >> 2, (u16 >> 2).astype(f32)),
                 (isp.load_32f, fl, fl)]
        for fn, src, x in cases:
            xw = O.cast_out(x * gain if g is not None else x, work)
            got = fn(torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
            assert_exact(got, ref_rgb(xw, m.mask(), work, O.GBRG, CCM), f"{cam} {fn.__name__} grid={g is not None}")
            assert_exact(fn(torch.from_numpy(src).to(dev)).cpu().numpy(), ref_rgb(xw, None, work, O.GBRG, CCM),
                         f"{cam} {fn.__name__} without a map")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_stuck_site_value_does_not_matter(ti, rng, dev, cam, work, H, W):
    """A site in the map gives the same outputs stuck at 4095 or at 0; without the map it does not."""
    r, c = H // 2, W // 2 + 1
    base = natural_packed12(rng, H, W, O.RGGB)
    codes = O.decode12(base, "u16")
    out = {}
    for v in (4095, 0):
        codes[r, c] = v
        out[v] = torch.from_numpy(O.encode12(codes)).to(dev)
    m = ti.DefectMap([[r, c]], (H, W))
    for rw in (0, W // 2):
        isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, resize_width=rw)
        hot, dead = (isp.load_packed12(out[v], defects=m).cpu().numpy() for v in (4095, 0))
        assert_exact(hot, dead, f"{cam} stuck site in the map, resize_width={rw}")
        hot, dead = (isp.load_packed12(out[v]).cpu().numpy() for v in (4095, 0))
        assert not np.array_equal(hot, dead), "without the map the stuck value shows"


@pytest.mark.parametrize("cam,work", CAMS)
def test_identity_cases(ti, rng, dev, cam, work):
    """Every site of one colour defective: no site has a usable neighbour, so the call gives the bits of the call
    without a map (every output pixel recomputed).  None and an empty map give today's bits."""
    for (H, W), rw in (((64, 256), 0), ((34, 130), 0), ((64, 256), 96)):
        raw = natural_packed12(rng, H, W, O.GBRG)
        t = torch.from_numpy(raw).to(dev)
        isp = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, resize_width=rw, correct_colors=True)
        plain = isp.load_packed12(t).cpu().numpy()
        every = np.zeros((H, W), bool)
        every[1::2, 0::2] = True
        for m in (ti.DefectMap.from_mask(every), None, ti.DefectMap([], (H, W))):
            assert_exact(isp.load_packed12(t, defects=m).cpu().numpy(), plain, f"{cam} {H}x{W} rw={rw} {m!r}")
        got = isp.load_packed12_batch([t, t], defects=[ti.DefectMap.from_mask(every), ti.DefectMap([], (H, W))])
        for g in got:
            assert_exact(g.cpu().numpy(), plain, f"{cam} batch identity")


def test_process_packed12_matches_two_calls(ti, rng, dev):
    H, W = 64, 256
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(4)]
    maps = [ti.DefectMap(defect_sites(H, W), (H, W)), None, ti.DefectMap([[5, 5], [40, 100]], (H, W)), None]
    a = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3)
    b = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3)
    for step in range(3):
        outs, imgs = a.process_packed12(frames, gamma=0.7, keep_images=True, defects=maps)
        ref_imgs = b.load_packed12_batch(frames, defects=maps)
        ref_outs = b.tonemap_reinhard(ref_imgs, gamma=0.7)
        for o, r in zip(outs, ref_outs):
            assert_exact(o.cpu().numpy(), r.cpu().numpy(), f"step {step} u8")
        for i, r in zip(imgs, ref_imgs):
            assert_exact(i.cpu().numpy(), r.cpu().numpy(), f"step {step} images")
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), f"step {step} metering state")
    with pytest.raises(ValueError):
        a.process_packed12(frames, defects=maps[:3])


@pytest.mark.parametrize("cam,work", CAMS)
def test_graph_capture_with_cached_map(ti, rng, dev, cam, work):
    H, W = 64, 256
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    m2 = ti.DefectMap([[3, 3], [33, 77]], (H, W))
    raw = natural_packed12(rng, H, W, O.RGGB)
    src = torch.from_numpy(raw).to(dev)
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev)
    eager = isp.load_packed12(src, defects=m).clone()
    eager_b = [x.clone() for x in isp.load_packed12_batch([src, src], defects=[m, m2])]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        isp.load_packed12(src, defects=m)                     # (warm-up on the capture stream)
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = isp.load_packed12(src, defects=m)
        outs = isp.load_packed12_batch([src, src], defects=[m, m2])
    g.replay()
    torch.cuda.synchronize(dev)
    assert_exact(out.cpu().numpy(), eager.cpu().numpy(), "captured load_packed12")
    for o, e in zip(outs, eager_b):
        assert_exact(o.cpu().numpy(), e.cpu().numpy(), "captured load_packed12_batch")
    ref = ref_rgb(cfa_x(raw, 12, work), m.mask(), work, O.RGGB)
    assert_exact(out.cpu().numpy(), ref, "captured against the oracle")
