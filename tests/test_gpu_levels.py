"""Sensor black and white levels (Camera16/32 black_level= / white_level=): every raw loader against the oracle.

Expected values come from the existing oracle without changing it: the raw codes (O.decode12 / O.decode16 unscaled), the
levels contract of DESIGN.md 3 in NumPy f32 - cast(f32(max(v - b_s, 0)) * k_s), k_s = f32(1 / (white - b_s)) - rounded to
the work dtype by O.cast_out, then O.bayer_to_rgb / O.resize_bilinear / O.metering_images / O.reinhard_isp as usual.
"""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests.util import _count_calls, assert_close, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
PER_SITE = [64, 200, 180, 256]


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def site_levels(black, H, W):
    b = np.broadcast_to(np.asarray(black if np.ndim(black) else [black] * 4, np.int64).reshape(2, 2), (2, 2))
    return np.tile(b, (H // 2, W // 2))


def apply_levels(codes, black, white, work):
    """The contract on raw codes (H, W) -> work-dtype CFA."""
    H, W = codes.shape
    b = site_levels(black, H, W)
    k = np.empty((2, 2), np.float32)
    bb = b[:2, :2]
    for i in range(2):
        for j in range(2):
            k[i, j] = np.float32(1.0 / (white - int(bb[i, j])))
    d = np.maximum(codes.astype(np.int64) - b, 0).astype(np.float32)
    return O.cast_out(d * np.tile(k, (H // 2, W // 2)), work)


def ref_load(packed, bits, work, pattern, black, white, resize_width=0, scale=None):
    codes = O.decode12(packed, "u16") if bits == 12 else O.decode16(packed, "u16")
    if bits == 12:
        white = 4095 if white is None else white
    else:
        white = 65535 if white is None else white
    black = 0 if black is None else black
    rgb = O.bayer_to_rgb(apply_levels(codes, black, white, work), pattern)
    sz = O.isp_output_size(rgb.shape[0], rgb.shape[1], resize_width, scale)
    return rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1])


def packed16(rng, H, W):
    v = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    v[0, :8] = [0, 1, 100, 300, 65535, 65534, 1000, 2000]       # codes below / above the black levels
    return v.view(np.uint8).reshape(H, 2 * W)


def with_dark_codes(packed):
    """A few 12-bit codes below the black levels (clamped to 0) at the start of the first row."""
    codes = O.decode12(packed, "u16")
    codes[0, :8] = [0, 3, 63, 64, 65, 199, 255, 4095]
    return O.encode12(codes)


# (H, W): the streaming kernel (W % 8 == 0), the tile kernel on a ragged width, a small odd-multiple frame
SHAPES = [(64, 256), (34, 130), (48, 104)]
LEVELS = [(64, None), (PER_SITE, None), (PER_SITE, 3900), (300, 4000)]


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("black,white", LEVELS)
def test_load_packed12_levels_bit_exact(ti, rng, dev, cam, work, shape, black, white):
    H, W = shape
    for p in range(4):
        packed = with_dark_codes(natural_packed12(rng, H, W, p))
        isp = getattr(ti, cam)(ti.BayerPattern(p), device=dev, black_level=black, white_level=white)
        got = isp.load_packed12(torch.from_numpy(packed).to(dev)).cpu().numpy()
        assert_exact(got, ref_load(packed, 12, work, p, black, white), f"{cam} {shape} p{p} {black}/{white}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("black,white", [(1000, None), (PER_SITE, 60000)])
def test_load_packed16_levels_bit_exact(ti, rng, dev, cam, work, black, white):
    for (H, W) in ((32, 128), (34, 130)):
        raw = packed16(rng, H, W)
        for p in range(4):
            isp = getattr(ti, cam)(ti.BayerPattern(p), device=dev, black_level=black, white_level=white)
            got = isp.load_packed16(torch.from_numpy(raw).to(dev)).cpu().numpy()
            assert_exact(got, ref_load(raw, 16, work, p, black, white), f"{cam} {H}x{W} p{p}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("black", [128, PER_SITE])
def test_load_packed_levels_with_resize(ti, rng, dev, cam, work, black):
    """A scale the fused kernel takes (0.5) and one it does not (resize separately: 0.25)."""
    H, W = 96, 256
    packed = with_dark_codes(natural_packed12(rng, H, W, O.GRBG))
    for rw in (128, 64, 200):
        isp = getattr(ti, cam)(ti.BayerPattern.GRBG, resize_width=rw, device=dev, black_level=black)
        got = isp.load_packed12(torch.from_numpy(packed).to(dev)).cpu().numpy()
        assert_exact(got, ref_load(packed, 12, work, O.GRBG, black, None, resize_width=rw), f"{cam} resize {rw}")
    raw = packed16(rng, 48, 128)
    isp = getattr(ti, cam)(ti.BayerPattern.GRBG, resize_width=64, device=dev, black_level=black, white_level=50000)
    assert_exact(isp.load_packed16(torch.from_numpy(raw).to(dev)).cpu().numpy(),
                 ref_load(raw, 16, work, O.GRBG, black, 50000, resize_width=64), f"{cam} packed16 resize")


@pytest.mark.parametrize("cam,work", CAMS)
def test_load_packed_batch_levels(ti, rng, dev, cam, work):
    for (H, W), rw in (((64, 256), 0), ((34, 130), 0), ((96, 256), 128)):
        frames = [with_dark_codes(natural_packed12(rng, H, W, O.BGGR, dark=0.1 * k)) for k in range(3)]
        isp = getattr(ti, cam)(ti.BayerPattern.BGGR, resize_width=rw, device=dev, black_level=PER_SITE, white_level=4000)
        got = isp.load_packed12_batch([torch.from_numpy(f).to(dev) for f in frames])
        for k, (g, f) in enumerate(zip(got, frames)):
            assert_exact(g.cpu().numpy(), ref_load(f, 12, work, O.BGGR, PER_SITE, 4000, resize_width=rw),
                         f"{cam} batch {H}x{W} frame {k}")
    raws = [packed16(rng, 32, 128) for _ in range(2)]
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, black_level=512)
    for g, r in zip(isp.load_packed16_batch([torch.from_numpy(r).to(dev) for r in raws]), raws):
        assert_exact(g.cpu().numpy(), ref_load(r, 16, work, O.RGGB, 512, None), f"{cam} batch16")


@pytest.mark.parametrize("cam,work", CAMS)
def test_load_16u_levels(ti, rng, dev, cam, work):
    """load_16u keeps its own division: cast(f32(max(v - b_s, 0)) / f32(white - b_s))."""
    raw = rng.integers(0, 65536, (34, 130), dtype=np.uint16)
    raw[0, :4] = [0, 10, 70000 % 65536, 65535]
    for black, white in ((PER_SITE, 60000), (2000, None)):
        isp = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=black, white_level=white)
        w = 65535 if white is None else white
        b = site_levels(black, 34, 130)
        d = np.maximum(raw.astype(np.int64) - b, 0).astype(np.float32)
        cfa = O.cast_out(d / (w - b).astype(np.float32), work)
        assert_exact(isp.load_16u(torch.from_numpy(raw).to(dev)).cpu().numpy(), O.bayer_to_rgb(cfa, O.GBRG), "load_16u")


@pytest.mark.parametrize("cam,work", CAMS)
def test_levels_metering_and_tonemap(ti, rng, dev, cam, work):
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, resize_width=64, device=dev, black_level=PER_SITE,
                           white_level=3900)
    st = O.IspState(0.3)
    for step in range(3):
        packs = [with_dark_codes(natural_packed12(rng, 80, 128, dark=0.05 * step)) for _ in range(3)]
        imgs = [isp.load_packed12(torch.from_numpy(p).to(dev)) for p in packs]
        refs = [ref_load(p, 12, work, O.RGGB, PER_SITE, 3900, resize_width=64) for p in packs]
        outs = isp.tonemap_reinhard(imgs, gamma=0.6)
        m = st.update_metering(refs)
        assert_close(isp.metrics.cpu().numpy(), m, f"metrics step {step}", rel=2e-5)
        for k, (o, r) in enumerate(zip(outs, refs)):
            assert_close(o.cpu().numpy(), O.reinhard_isp(r, m, gamma=0.6)[0], f"u8 step {step} img {k}")


@pytest.mark.parametrize("pattern,black", [(O.RGGB, PER_SITE), (O.GBRG, 128)])
def test_process_packed12_levels_4k_fused(ti, dev, monkeypatch, pattern, black):
    """A 4096 x 3072 camera group with levels through the fused camera-group path (checked: the call reaches
    mi_isp_camera_group_reinhard_levels): the same u8 outputs, mapped images and metering state, bit for bit, as
    load_packed12_batch + tonemap_reinhard with the same levels, and the oracle chain within the parity tolerances."""
    from taichi_image_amd import synthetic
    H, W = 3072, 4096
    frames = [synthetic.synthetic_packed12(k, H, W) for k in range(2)]
    kw = dict(moving_alpha=0.5, device=dev, black_level=black, white_level=4000)
    a, b = ti.Camera16(ti.BayerPattern(pattern), **kw), ti.Camera16(ti.BayerPattern(pattern), **kw)
    fused_calls = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard_levels")
    st = O.IspState(0.5)
    for step in range(2):
        dframes = [torch.from_numpy(f).to(dev) for f in frames]
        outs, imgs = a.process_packed12(dframes, gamma=0.6, keep_images=True)
        assert len(fused_calls) == step + 1, "process_packed12 with levels did not take the camera-group kernel"
        imgs_b = b.load_packed12_batch(dframes)
        outs_b = b.tonemap_reinhard(imgs_b, gamma=0.6)
        assert torch.equal(a.metrics, b.metrics), f"metering state, step {step}"
        for k in range(len(frames)):
            assert torch.equal(outs[k], outs_b[k]), f"u8 output {k}, step {step}"
            assert torch.equal(imgs[k].view(torch.int16), imgs_b[k].view(torch.int16)), f"image (p) {k}, step {step}"
        refs = [ref_load(f, 12, "f16", pattern, black, 4000) for f in frames]
        m = st.update_metering(refs)
        assert_close(a.metrics.cpu().numpy(), m, f"metrics vs oracle, step {step}", rel=2e-5)
        assert_close(outs[0].cpu().numpy(), O.reinhard_isp(refs[0], m, gamma=0.6)[0], f"u8 vs oracle, step {step}")
        frames = frames[::-1]


def test_process_packed12_levels_identity_4k_fused(ti, dev, monkeypatch):
    """black_level=0 on the fused camera-group path: bit-identical to the same path without levels."""
    from taichi_image_amd import synthetic
    frames = [torch.from_numpy(synthetic.synthetic_packed12(k, 3072, 4096)).to(dev) for k in range(2)]
    x = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev)
    y = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev, black_level=0)
    plain = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard")
    with_levels = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard_levels")
    for _ in range(2):
        ox, oy = x.process_packed12(frames, gamma=0.6), y.process_packed12(frames, gamma=0.6)
        assert torch.equal(x.metrics, y.metrics)
        assert all(torch.equal(a, b) for a, b in zip(ox, oy))
    assert len(plain) == 2 and len(with_levels) == 2


@pytest.mark.parametrize("cam,work", CAMS)
def test_levels_identity(ti, rng, dev, cam, work):
    """black_level=0 with the default white level: bit-identical to no levels on every loader."""
    def pair(**kw):
        return (getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, **kw),
                getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=0, **kw))
    cases = [((64, 256), {}), ((34, 130), {}), ((96, 256), {"resize_width": 128}), ((96, 256), {"resize_width": 64})]
    for (H, W), kw in cases:
        packed = torch.from_numpy(natural_packed12(rng, H, W, O.GBRG)).to(dev)
        x, y = pair(**kw)
        assert torch.equal(x.load_packed12(packed).view(torch.int16), y.load_packed12(packed).view(torch.int16)), (H, W, kw)
        for gx, gy in zip(x.load_packed12_batch([packed, packed]), y.load_packed12_batch([packed, packed])):
            assert torch.equal(gx.view(torch.int16), gy.view(torch.int16))
    raw = torch.from_numpy(packed16(rng, 34, 130)).to(dev)
    x, y = pair()
    assert torch.equal(x.load_packed16(raw), y.load_packed16(raw))
    u16 = torch.from_numpy(rng.integers(0, 65536, (34, 130), dtype=np.uint16)).to(dev)
    assert torch.equal(x.load_16u(u16), y.load_16u(u16))
    frames = [torch.from_numpy(natural_packed12(rng, 64, 256, O.GBRG, dark=0.1 * k)).to(dev) for k in range(2)]
    if work == "f16":
        ox, oy = x.process_packed12(frames, gamma=0.6), y.process_packed12(frames, gamma=0.6)
        assert torch.equal(x.metrics, y.metrics)
        assert all(torch.equal(a, b) for a, b in zip(ox, oy))


def test_levels_validation(ti, rng, dev):
    with pytest.raises(ValueError):
        ti.Camera16(ti.BayerPattern.RGGB, device=dev, black_level=-1)
    with pytest.raises(ValueError):
        ti.Camera16(ti.BayerPattern.RGGB, device=dev, black_level=[1, 2, 3])
    with pytest.raises(ValueError):
        ti.Camera16(ti.BayerPattern.RGGB, device=dev, black_level=64.0)
    with pytest.raises(ValueError):
        ti.Camera16(ti.BayerPattern.RGGB, device=dev, black_level=500, white_level=500)
    with pytest.raises(ValueError):
        ti.Camera16(ti.BayerPattern.RGGB, device=dev, white_level=70000)
    packed = torch.from_numpy(natural_packed12(rng, 64, 256)).to(dev)
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev)
    isp.tonemap_reinhard([isp.load_packed12(packed)])
    before = isp.metrics.clone()
    with pytest.raises(ValueError):
        isp.set(black_level=[0, 0, 0, 70000])
    assert isp.black_level is None
    isp.set(white_level=8000)                      # fine for a 16-bit source, not for packed-12
    with pytest.raises(ValueError):
        isp.load_packed12(packed)
    with pytest.raises(ValueError):
        isp.process_packed12([packed])
    assert torch.equal(isp.metrics, before)
    isp.set(white_level=4095, black_level=64)
    with pytest.raises(ValueError):
        isp.load_16f(torch.zeros((8, 8), dtype=torch.uint16, device=dev))
    with pytest.raises(ValueError):
        isp.load_32f(torch.zeros((8, 8), dtype=torch.float32, device=dev))
    assert torch.equal(isp.metrics, before)


def test_scan_cli_black_level(tmp_path):
    from taichi_image_amd.scripts import tonemap_scan as ts
    from tests.test_tonemap_scan import _read_png
    H, W = 34, 130
    frames = {}
    for c, cam in enumerate(("cam0", "cam1")):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        frames[cam] = with_dark_codes(natural_packed12(np.random.default_rng(c), H, W, dark=0.1 * c))
        (tmp_path / "scan" / cam / "frame0.raw").write_bytes(frames[cam].tobytes())
    out = tmp_path / "out"
    assert ts.main(["--scan", str(tmp_path / "scan"), "--width", str(W), "--write", str(out), "--rows", "1",
                    "--black-level", *map(str, PER_SITE), "--white-level", "4000"]) == 0
    refs = [ref_load(frames[cam], 12, "f32", O.RGGB, PER_SITE, 4000) for cam in ("cam0", "cam1")]
    m = O.IspState(0.02).update_metering(refs)
    want = np.concatenate([O.transform(O.reinhard_isp(r, m, gamma=0.9, intensity=3.0, light_adapt=0.9, color_adapt=0.0)[0],
                                       "rotate_90") for r in refs], axis=1)
    assert_close(_read_png(out / "frame0.png"), want, "scan with levels")
    with pytest.raises(ValueError):
        ts.main(["--scan", str(tmp_path / "scan"), "--black-level", "5000"])
