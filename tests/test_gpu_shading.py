"""Lens shading (Camera16/32 lens_shading=): every raw loader against the oracle.

Expected values come from the existing oracle without changing it: the raw codes (O.decode12 / O.decode16 unscaled), the
levels and the shading contract of DESIGN.md 3 in NumPy f32 (every operation rounded, nothing fused), rounded to the
work dtype by O.cast_out, then O.bayer_to_rgb / O.resize_bilinear / O.metering_images / O.reinhard_isp as usual.
"""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests.util import _count_calls, assert_close, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
PER_SITE = [64, 200, 180, 256]
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_grid(rng, gh, gw, sites):
    """A vignetting-like grid (larger gains toward the corners) with per-node noise, f32."""
    y = np.linspace(-1, 1, gh)[:, None]
    x = np.linspace(-1, 1, gw)[None, :]
    g = np.stack([1.0 + (0.6 + 0.1 * s) * (y * y + x * x) / 2 + rng.uniform(-0.05, 0.05, (gh, gw)) for s in range(sites)])
    return (g[0] if sites == 1 else g).astype(f32)


def pixel_gains(grid, H, W):
    """The contract: the gain of every raw pixel, (H, W) f32."""
    g3 = grid[None] if grid.ndim == 2 else grid
    _, gh, gw = g3.shape
    sy = f32((gh - 1) / (H - 1)) if H > 1 else f32(0)
    sx = f32((gw - 1) / (W - 1)) if W > 1 else f32(0)
    v = np.arange(H).astype(f32) * sy
    i = np.minimum(np.floor(v).astype(np.int64), gh - 2)
    ty = (v - i.astype(f32))[:, None]
    u = np.arange(W).astype(f32) * sx
    j = np.minimum(np.floor(u).astype(np.int64), gw - 2)
    tx = (u - j.astype(f32))[None, :]
    out = np.empty((H, W), f32)
    site = (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)
    for s in range(g3.shape[0]):
        G = g3[s]
        g00, g10 = G[i][:, j], G[i + 1][:, j]
        g01, g11 = G[i][:, j + 1], G[i + 1][:, j + 1]
        a = g00 + ty * (g10 - g00)
        b = g01 + ty * (g11 - g01)
        g = a + tx * (b - a)
        if g3.shape[0] == 1:
            return g
        out[site == s] = g[site == s]
    return out


def site_levels(black, H, W):
    b = np.asarray(black if np.ndim(black) else [black] * 4, np.int64).reshape(2, 2)
    return np.tile(b, (H // 2, W // 2))


def raw_x(codes, bits, black, white):
    """The f32 value the loader rounds to the work dtype without shading (levels included)."""
    H, W = codes.shape
    if black is None and white is None:
        return codes.astype(f32) * f32(1.0 / (4095.0 if bits == 12 else 65535.0))
    white = ((1 << bits) - 1) if white is None else white
    b = site_levels(0 if black is None else black, H, W)
    k = np.empty((2, 2), f32)
    for r in range(2):
        for c in range(2):
            k[r, c] = f32(1.0 / (white - int(b[r, c])))
    return np.maximum(codes.astype(np.int64) - b, 0).astype(f32) * np.tile(k, (H // 2, W // 2))


def ref_load(raw, bits, work, pattern, grid, black=None, white=None, resize_width=0, ids_format=False, ccm=None):
    codes = O.decode12(raw, "u16", ids_format=ids_format) if bits == 12 else O.decode16(raw, "u16")
    x = raw_x(codes, bits, black, white)
    if grid is not None:
        x = x * pixel_gains(grid, *codes.shape)
    rgb = O.bayer_to_rgb(O.cast_out(x, work), pattern, correct_colors=ccm)
    sz = O.isp_output_size(rgb.shape[0], rgb.shape[1], resize_width, None)
    return rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1])


def packed16(rng, H, W):
    return rng.integers(0, 65536, (H, W), dtype=np.uint16).view(np.uint8).reshape(H, 2 * W)


GRIDS = [(2, 2), (17, 13), (33, 33), (64, 2)]
SHAPES = [(64, 256), (34, 130)]                     # streaming width (W % 8 == 0), ragged tile width
LEVELS = [(None, None), (PER_SITE, 3900)]


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("gshape", GRIDS)
@pytest.mark.parametrize("sites", [1, 4])
@pytest.mark.parametrize("black,white", LEVELS)
def test_load_packed12_shading_bit_exact(ti, rng, dev, cam, work, gshape, sites, black, white):
    grid = make_grid(rng, *gshape, sites)
    for (H, W) in SHAPES:
        for p in (O.RGGB, O.GBRG):
            packed = natural_packed12(rng, H, W, p)
            isp = getattr(ti, cam)(ti.BayerPattern(p), device=dev, black_level=black, white_level=white,
                                   lens_shading=grid)
            got = isp.load_packed12(torch.from_numpy(packed).to(dev)).cpu().numpy()
            assert_exact(got, ref_load(packed, 12, work, p, grid, black, white), f"{cam} {H}x{W} p{p} grid {grid.shape}")
            # IDS layout: the tile kernel's general fill
            ids = natural_packed12(rng, H, W, p, ids_format=True)
            got = isp.load_packed12(torch.from_numpy(ids).to(dev), ids_format=True).cpu().numpy()
            assert_exact(got, ref_load(ids, 12, work, p, grid, black, white, ids_format=True), f"{cam} IDS {H}x{W}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("sites", [1, 4])
def test_load_packed16_shading(ti, rng, dev, cam, work, sites):
    grid = make_grid(rng, 17, 13, sites)
    for (H, W) in ((32, 128), (34, 130)):
        raw = packed16(rng, H, W)
        for black, white in ((None, None), (PER_SITE, 60000)):
            isp = getattr(ti, cam)(ti.BayerPattern.GRBG, device=dev, black_level=black, white_level=white,
                                   lens_shading=grid)
            got = isp.load_packed16(torch.from_numpy(raw).to(dev)).cpu().numpy()
            assert_exact(got, ref_load(raw, 16, work, O.GRBG, grid, black, white), f"{cam} packed16 {H}x{W} {black}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("black", [None, PER_SITE])
def test_load_packed_shading_with_resize(ti, rng, dev, cam, work, black):
    """The fused resize (stream kernel on Camera16, resize tile kernel on Camera32) and a scale it does not take."""
    H, W = 96, 256
    packed = natural_packed12(rng, H, W, O.GRBG)
    for gshape, sites in (((33, 33), 4), ((2, 2), 1), ((64, 2), 4)):
        grid = make_grid(rng, *gshape, sites)
        for rw in (128, 64, 200):
            isp = getattr(ti, cam)(ti.BayerPattern.GRBG, resize_width=rw, device=dev, black_level=black, lens_shading=grid)
            got = isp.load_packed12(torch.from_numpy(packed).to(dev)).cpu().numpy()
            assert_exact(got, ref_load(packed, 12, work, O.GRBG, grid, black, None, resize_width=rw), f"{cam} resize {rw}")


@pytest.mark.parametrize("cam,work", CAMS)
def test_load_packed12_batch_shading(ti, rng, dev, cam, work):
    """More than 8 frames (two batched launches), with and without resize; the metering subsample on the way."""
    grid = make_grid(rng, 17, 13, 4)
    for (H, W), rw in (((64, 256), 0), ((34, 130), 0), ((96, 256), 128)):
        frames = [natural_packed12(rng, H, W, O.BGGR, dark=0.02 * k) for k in range(10)]
        isp = getattr(ti, cam)(ti.BayerPattern.BGGR, resize_width=rw, device=dev, black_level=PER_SITE, white_level=4000,
                               lens_shading=grid)
        got = isp.load_packed12_batch([torch.from_numpy(f).to(dev) for f in frames])
        for k, (g, f) in enumerate(zip(got, frames)):
            ref = ref_load(f, 12, work, O.BGGR, grid, PER_SITE, 4000, resize_width=rw)
            assert_exact(g.cpu().numpy(), ref, f"{cam} batch {H}x{W} frame {k}")
            sub = getattr(g, "_mi_metering_sub", None)
            if sub is not None:
                assert_exact(sub[0].cpu().numpy(), ref[::8, ::8],
                             "metering subsample")


@pytest.mark.parametrize("cam,work", CAMS)
def test_full_size_shading(ti, rng, dev, cam, work):
    from taichi_image_amd import synthetic
    packed = synthetic.synthetic_packed12(3, 3072, 4096)
    grid = make_grid(rng, 17, 13, 4)
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, black_level=PER_SITE, lens_shading=grid)
    got = isp.load_packed12(torch.from_numpy(packed).to(dev)).cpu().numpy()
    assert_exact(got, ref_load(packed, 12, work, O.RGGB, grid, PER_SITE), f"{cam} 4096x3072")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("sites", [1, 4])
def test_load_convert_shading(ti, rng, dev, cam, work, sites):
    grid = make_grid(rng, 33, 33, sites)
    H, W = 34, 130
    g = pixel_gains(grid, H, W)
    u16 = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    u16f = rng.integers(0, 30000, (H, W), dtype=np.uint16)     # (load_16f: times a gain < 2, still finite in f16)
    fl = rng.random((H, W), dtype=np.float32)
    isp = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, lens_shading=grid)
    cases = [(isp.load_16u, u16, u16.astype(f32) / f32(65535.0)), (isp.load_16f, u16f, u16f.astype(f32)),
             (isp.load_32f, fl, fl)]
    for fn, src, x in cases:
        got = fn(torch.from_numpy(src).to(dev)).cpu().numpy()
        assert_exact(got, O.bayer_to_rgb(O.cast_out(x * g, work), O.GBRG), f"{cam} {fn.__name__}")
    isp.set(black_level=PER_SITE, white_level=60000)
    b = site_levels(PER_SITE, H, W)
    x = np.maximum(u16.astype(np.int64) - b, 0).astype(f32) / (60000 - b).astype(f32)
    got = isp.load_16u(torch.from_numpy(u16).to(dev)).cpu().numpy()
    assert_exact(got, O.bayer_to_rgb(O.cast_out(x * g, work), O.GBRG), f"{cam} load_16u with levels")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("black", [None, PER_SITE])
def test_shading_identity(ti, rng, dev, cam, work, black):
    """A grid of ones is bit-identical to no shading on every loader."""
    for gshape, sites in (((2, 2), 1), ((17, 13), 4)):
        ones = np.ones(gshape if sites == 1 else (4,) + gshape, f32)
        for (H, W), kw in (((64, 256), {}), ((34, 130), {}), ((96, 256), {"resize_width": 128}),
                           ((96, 256), {"resize_width": 64})):
            x = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=black, **kw)
            y = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=black, lens_shading=ones, **kw)
            packed = torch.from_numpy(natural_packed12(rng, H, W, O.GBRG)).to(dev)
            assert torch.equal(x.load_packed12(packed).view(torch.int16), y.load_packed12(packed).view(torch.int16))
            for gx, gy in zip(x.load_packed12_batch([packed] * 3), y.load_packed12_batch([packed] * 3)):
                assert torch.equal(gx.view(torch.int16), gy.view(torch.int16))
        x = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=black)
        y = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=black, lens_shading=ones)
        raw = torch.from_numpy(packed16(rng, 34, 130)).to(dev)
        assert torch.equal(x.load_packed16(raw), y.load_packed16(raw))
        u16 = torch.from_numpy(rng.integers(0, 65536, (34, 130), dtype=np.uint16)).to(dev)
        assert torch.equal(x.load_16u(u16), y.load_16u(u16))
        if black is None:
            assert torch.equal(x.load_16f(u16), y.load_16f(u16))
            fl = torch.rand((34, 130), device=dev)
            assert torch.equal(x.load_32f(fl), y.load_32f(fl))


@pytest.mark.parametrize("cam,work", CAMS)
def test_shading_metering_and_tonemap(ti, rng, dev, cam, work):
    grid = make_grid(rng, 17, 13, 4)
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, resize_width=64, device=dev, black_level=PER_SITE,
                           white_level=3900, lens_shading=grid)
    st = O.IspState(0.3)
    for step in range(3):
        packs = [natural_packed12(rng, 80, 128, dark=0.05 * step) for _ in range(3)]
        imgs = [isp.load_packed12(torch.from_numpy(p).to(dev)) for p in packs]
        refs = [ref_load(p, 12, work, O.RGGB, grid, PER_SITE, 3900, resize_width=64) for p in packs]
        outs = isp.tonemap_reinhard(imgs, gamma=0.6)
        m = st.update_metering(refs)
        assert_close(isp.metrics.cpu().numpy(), m, f"metrics step {step}", rel=2e-5)
        for k, (o, r) in enumerate(zip(outs, refs)):
            assert_close(o.cpu().numpy(), O.reinhard_isp(r, m, gamma=0.6)[0], f"u8 step {step} img {k}")


def test_process_packed12_shading_4k(ti, rng, dev, monkeypatch):
    """With a grid, process_packed12 takes the two calls (load_packed12_batch + tonemap_reinhard), not the camera group."""
    from taichi_image_amd import synthetic
    frames = [torch.from_numpy(synthetic.synthetic_packed12(k, 3072, 4096)).to(dev) for k in range(2)]
    grid = make_grid(rng, 17, 13, 4)
    kw = dict(moving_alpha=0.5, device=dev, lens_shading=grid)
    a, b = ti.Camera16(ti.BayerPattern.RGGB, **kw), ti.Camera16(ti.BayerPattern.RGGB, **kw)
    group = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard")
    group_lv = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard_levels")
    for step in range(2):
        outs, imgs = a.process_packed12(frames, gamma=0.6, keep_images=True)
        imgs_b = b.load_packed12_batch(frames)
        outs_b = b.tonemap_reinhard(imgs_b, gamma=0.6)
        assert torch.equal(a.metrics, b.metrics), f"metering state, step {step}"
        for k in range(len(frames)):
            assert torch.equal(outs[k], outs_b[k]), f"u8 output {k}, step {step}"
            assert torch.equal(imgs[k].view(torch.int16), imgs_b[k].view(torch.int16)), f"image {k}, step {step}"
        frames = frames[::-1]
    assert not group and not group_lv, "process_packed12 with a grid took the camera-group kernel"


def test_grid_update_between_loads(ti, rng, dev):
    """set(lens_shading=...) between two loads on one stream changes the second output only (same shape: in place;
    another shape: a new grid); False removes the grid."""
    H, W = 64, 256
    packed = natural_packed12(rng, H, W)
    d = torch.from_numpy(packed).to(dev)
    g1, g2, g3 = make_grid(rng, 17, 13, 4), make_grid(rng, 17, 13, 4), make_grid(rng, 5, 9, 1)
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, lens_shading=g1)
    first = isp.load_packed12(d)
    isp.set(lens_shading=g2)
    second = isp.load_packed12(d)
    isp.set(lens_shading=torch.from_numpy(g3))
    third = isp.load_packed12(d)
    isp.set(lens_shading=None)                     # leaves the grid
    fourth = isp.load_packed12(d)
    isp.set(lens_shading=False)
    fifth = isp.load_packed12(d)
    torch.cuda.synchronize()
    assert_exact(first.cpu().numpy(), ref_load(packed, 12, "f16", O.RGGB, g1), "before the update")
    assert_exact(second.cpu().numpy(), ref_load(packed, 12, "f16", O.RGGB, g2), "after the update")
    assert_exact(third.cpu().numpy(), ref_load(packed, 12, "f16", O.RGGB, g3), "after a new shape")
    assert_exact(fourth.cpu().numpy(), ref_load(packed, 12, "f16", O.RGGB, g3), "set(None)")
    assert_exact(fifth.cpu().numpy(), ref_load(packed, 12, "f16", O.RGGB, None), "removed")
    assert isp.lens_shading is None


def test_calibration_round_trip(ti, dev):
    from taichi_image_amd import camera_isp
    H, W, gh, gw = 768, 1024, 13, 17
    rr, cc = np.mgrid[0:H, 0:W].astype(np.float64)
    ry, rx = (rr - (H - 1) / 2) / (H / 2), (cc - (W - 1) / 2) / (W / 2)
    site = (rr.astype(int) & 1) * 2 + (cc.astype(int) & 1)
    g_true = np.stack([1.0 + (0.3 + 0.05 * s) * (ry * ry + rx * rx) / 2 for s in range(4)])
    base = np.array([3000.0, 2600.0, 2600.0, 3200.0])        # (the green sites alike: one flat G channel)
    flat = np.round(np.choose(site, base) / np.choose(site, g_true)).astype(np.uint16)
    grid = camera_isp.lens_shading_from_flat(torch.from_numpy(flat.astype(np.int32)).to(dev), (gh, gw))
    assert grid.device.type == "cuda" and grid.shape == (4, gh, gw)
    ys, xs = np.arange(gh) * (H - 1) / (gh - 1), np.arange(gw) * (W - 1) / (gw - 1)
    for s in range(4):
        t = 1.0 + (0.3 + 0.05 * s) * (((ys[:, None] - (H - 1) / 2) / (H / 2)) ** 2 +
                                      ((xs[None, :] - (W - 1) / 2) / (W / 2)) ** 2) / 2
        rel = np.abs(grid[s].cpu().numpy() / (t / t.min()) - 1)
        assert rel[1:-1, 1:-1].max() < 0.02 and rel.max() < 0.03, (s, rel.max())
    # the flat through the loader with that grid: every channel of the demosaiced image flat within 3 % (max / min)
    isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev, lens_shading=grid)
    u16 = torch.from_numpy(flat).to(dev)
    codes = (isp.load_16u(u16) * 65535.0).cpu().numpy()    # the demosaiced image of a corrected flat
    for ch in range(3):
        v = codes[4:-4, 4:-4, ch]
        assert v.max() / v.min() < 1.03, (ch, v.max() / v.min())
    # a flat constant per site gives exact ones
    const = np.choose(site, base).astype(np.uint16)
    assert np.all(camera_isp.lens_shading_from_flat(const, (gh, gw)) == 1.0)


def test_scan_cli_lens_shading(tmp_path, rng):
    from taichi_image_amd.scripts import tonemap_scan as ts
    from tests.test_tonemap_scan import _read_png
    H, W = 34, 130
    grid = make_grid(rng, 9, 7, 4)
    np.save(tmp_path / "grid.npy", grid)
    frames = {}
    for c, cam in enumerate(("cam0", "cam1")):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        frames[cam] = natural_packed12(np.random.default_rng(c), H, W, dark=0.1 * c)
        (tmp_path / "scan" / cam / "frame0.raw").write_bytes(frames[cam].tobytes())
    out = tmp_path / "out"
    assert ts.main(["--scan", str(tmp_path / "scan"), "--width", str(W), "--write", str(out), "--rows", "1",
                    "--lens-shading", str(tmp_path / "grid.npy")]) == 0
    refs = [ref_load(frames[cam], 12, "f32", O.RGGB, grid) for cam in ("cam0", "cam1")]
    m = O.IspState(0.02).update_metering(refs)
    want = np.concatenate([O.transform(O.reinhard_isp(r, m, gamma=0.9, intensity=3.0, light_adapt=0.9, color_adapt=0.0)[0],
                                       "rotate_90") for r in refs], axis=1)
    assert_close(_read_png(out / "frame0.png"), want, "scan with lens shading")
    np.save(tmp_path / "bad.npy", np.full((3, 3), 20.0, f32))
    with pytest.raises(ValueError):
        ts.main(["--scan", str(tmp_path / "scan"), "--lens-shading", str(tmp_path / "bad.npy")])
