"""Raw noise reduction (Camera16/32 raw_denoise=, denoise_cfa) on the GPU against tests/denoise_ref.py.

The route's CFA is captured by wrapping ISP._process_image; it must hold the stated bound against the f64 contract
(denoise_ref.assert_within_bound) at every unlisted site and the defect fix-up's bits at every listed one, and the loader's
image must be O.bayer_to_rgb / O.resize_bilinear of that CFA bit for bit."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import denoise_ref as D
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_defects import defect_sites
from tests.test_gpu_shading import PER_SITE, make_grid, packed16, pixel_gains, raw_x
from tests.util import assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
CCM = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
f32 = np.float32
DN = {1: None, 2: None}


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    DN[1] = t.RawDenoise(0.002, 0.01, strength=1.5, radius=1)
    DN[2] = t.RawDenoise(0.002, 0.01, strength=1.0, radius=2, spatial_sigma=1.5)
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def capture(monkeypatch, isp):
    """The CFAs the route hands to _process_image, in call order."""
    got = []
    cls = type(isp)
    orig = cls._process_image

    def wrapped(self, cfa, lens=None):
        got.append(cfa.clone())
        return orig(self, cfa, lens)

    monkeypatch.setattr(cls, "_process_image", wrapped)
    return got


def noisy_cfa(rng, H, W, work):
    x = 0.05 + 0.8 * rng.random((H, W)) ** 2
    x = np.where(rng.random((H, W)) < 0.3, x, 0.4 + rng.normal(0, 0.02, (H, W)))    # flat patches and texture
    return O.cast_out(x.astype(f32), work)


# ---- denoise_cfa -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("H,W", [(64, 256), (34, 130), (67, 129), (130, 66), (2, 2), (4, 6), (1, 5), (3, 1)])
def test_denoise_cfa_bound(ti, rng, dev, work, radius, H, W):
    x = noisy_cfa(rng, H, W, work)
    dn = DN[radius]
    got = ti.denoise.denoise_cfa(torch.from_numpy(x).to(dev), dn)
    assert got.device == dev and got.dtype == torch.from_numpy(x).dtype and got.shape == (H, W)
    D.assert_within_bound(got.cpu().numpy(), D.filter_x(x, dn), work, f"{work} R={radius} {H}x{W}")
    host = ti.denoise.denoise_cfa(x, dn)                              # numpy in, numpy out
    assert isinstance(host, np.ndarray)
    assert_exact(host, got.cpu().numpy(), "numpy round trip")


@pytest.mark.parametrize("work,radius", [("f16", 1), ("f32", 2)])
def test_denoise_cfa_4k(ti, rng, dev, work, radius):
    x = noisy_cfa(rng, 3072, 4096, work)
    got = ti.denoise.denoise_cfa(torch.from_numpy(x).to(dev), DN[radius]).cpu().numpy()
    D.assert_within_bound(got, D.filter_x(x, DN[radius]), work, f"4K {work} R={radius}")


def test_denoise_cfa_flat_and_identity(ti, rng, dev):
    for work in ("f16", "f32"):
        x = O.cast_out(np.full((40, 70), 0.37, f32), work)
        assert_exact(ti.denoise.denoise_cfa(x, DN[2]), x, f"flat {work}")
        y = noisy_cfa(rng, 40, 70, work)
        assert_exact(ti.denoise.denoise_cfa(y, ti.RawDenoise(0.002, 0.01, spatial_sigma=0.05, radius=2)), y, "identity")
    with pytest.raises(ValueError):
        ti.denoise.denoise_cfa(np.zeros((8, 8), np.uint16), DN[1])


# ---- the loaders -------------------------------------------------------------------------------------------------------
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]


def make_source(rng, kind, H, W):
    """(the loader's input as numpy, its x as the loader computes it (levels applied by the caller's raw_x))."""
    if kind in ("p12", "ids"):
        raw = natural_packed12(rng, H, W, O.RGGB, ids_format=kind == "ids")
        return raw, O.decode12(raw, "u16", ids_format=kind == "ids")
    if kind == "p16":
        raw = packed16(rng, H, W)
        return raw, O.decode16(raw, "u16")
    u = (rng.random((H, W)) * 0.6 + 0.2 + rng.normal(0, 0.02, (H, W))).clip(0, 1)
    if kind == "16u":
        c = np.rint(u * 65535).astype(np.uint16)
        return c, c
    if kind == "16f":
        c = np.rint(u * 1000).astype(np.uint16)
        return c, c
    return u.astype(f32), u.astype(f32)


def loader_x(kind, codes, black, white):
    if kind in ("p12", "ids", "p16"):
        return raw_x(codes, 12 if kind != "p16" else 16, black, white)
    if kind == "16u":
        if black is None:
            return codes.astype(f32) / f32(65535.0)
        b = np.tile(np.reshape(black, (2, 2)), (codes.shape[0] // 2, codes.shape[1] // 2))
        den = (white - b).astype(f32)
        return np.maximum(codes.astype(np.int64) - b, 0).astype(f32) / den
    return codes.astype(f32)


def call(isp, kind, t, **kw):
    if kind == "p16":
        return isp.load_packed16(t, **kw)
    if kind in ("p12", "ids"):
        return isp.load_packed12(t, ids_format=kind == "ids", **kw)
    return {"16u": isp.load_16u, "16f": isp.load_16f, "32f": isp.load_32f}[kind](t, **kw)


CONFIGS = [
    dict(),                                                                     # plain
    dict(levels=True, grid=True),                                               # per-site levels + a per-site grid
    dict(awb=True, resize_width=96),                                            # AWB gains, the resize
    dict(grid=True, defects=True, radius=2),                                    # listed defects, radius 2
]


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_loaders_against_the_contract(ti, rng, dev, monkeypatch, cam, work, kind, cfg):
    c = CONFIGS[cfg]
    H, W = 66, 260
    src, codes = make_source(rng, kind, H, W)
    levels = c.get("levels") and kind in ("p12", "ids", "p16", "16u")
    black, white = (PER_SITE, 3900) if levels else (None, None)
    grid = make_grid(rng, 9, 13, 4) if c.get("grid") else None
    dn = DN[c.get("radius", 1)]
    mask = None
    kw = {}
    if c.get("defects"):
        m = ti.DefectMap(defect_sites(H, W), (H, W))
        mask = m.mask()
        kw["defects"] = m
    isp = getattr(ti, cam)(ti.BayerPattern.GRBG, device=dev, correct_colors=True, color_correction=CCM,
                           black_level=black, white_level=white, lens_shading=grid, raw_denoise=dn,
                           resize_width=c.get("resize_width", 0), auto_white_balance=bool(c.get("awb")))
    gain = None
    if isp._applied_shading() is not None:
        gain = pixel_gains(isp._applied_shading().cpu().numpy(), H, W)
    got_cfa = capture(monkeypatch, isp)
    img = call(isp, kind, torch.from_numpy(src).to(dev), **kw).cpu().numpy()
    cfa = got_cfa[0].cpu().numpy()
    x = loader_x(kind, codes, black, white)
    what = f"{cam} {kind} {c}"
    listed = np.zeros((H, W), bool) if mask is None else mask
    D.assert_within_bound(cfa, D.route_yg(x, dn, gain, mask), work, what, where=~listed)
    if mask is not None:
        assert_exact(cfa, correct_cfa(cfa, mask, work), what + " defect fix-up")
    rgb = O.bayer_to_rgb(cfa, O.GRBG, correct_colors=isp.color_correct_matrix)
    sz = O.isp_output_size(H, W, isp.resize_width, None)
    assert_exact(img, rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1]), what + " image")


def _identity_isps(ti, dev, cam, **kw):
    off = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, correct_colors=True, **kw)
    on = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, correct_colors=True,
                          raw_denoise=ti.RawDenoise(0.002, 0.01, radius=2, spatial_sigma=0.05), **kw)
    return off, on


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_identity_is_bit_exact(ti, rng, dev, cam, work, kind):
    """spatial_sigma = 0.05: every loader gives the bits of the same call without denoise, with levels, shading, AWB,
    defects, the resize and a lens."""
    H, W = 64, 256
    src, _ = make_source(rng, kind, H, W)
    t = torch.from_numpy(src).to(dev)
    lv = kind in ("p12", "ids", "p16", "16u")
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    K = np.array([[200.0, 0, W / 2 - 3], [0, 210.0, H / 2 + 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, (-0.2, 0.05, 0.001, -0.002), (H, W))
    cases = [dict(isp={}, call={}),
             dict(isp=dict(black_level=PER_SITE if lv else None, white_level=3900 if lv else None,
                           lens_shading=make_grid(rng, 5, 7, 4)), call={}),
             dict(isp=dict(auto_white_balance=True, resize_width=96), call=dict(defects=m)),
             dict(isp=dict(lens_shading=make_grid(rng, 3, 3, 1), scale=0.5), call=dict(defects=m, undistort=lens))]
    if kind in ("p12", "p16"):
        cases.append(dict(isp=dict(scale=0.37), call={}))              # a scale the fused resize does not take
    for case in cases:
        off, on = _identity_isps(ti, dev, cam, **case["isp"])
        for step in range(2):
            a = call(off, kind, t, **case["call"])
            b = call(on, kind, t, **case["call"])
            assert_exact(b.cpu().numpy(), a.cpu().numpy(), f"{cam} {kind} {case['isp']} {list(case['call'])} step {step}")
            off.tonemap_reinhard([a], gamma=0.9)
            on.tonemap_reinhard([b], gamma=0.9)
            assert_exact(on.metrics.cpu().numpy(), off.metrics.cpu().numpy(), "metering")
    # the batch forms
    if kind in ("p12", "p16"):
        off, on = _identity_isps(ti, dev, cam, resize_width=96)
        fn = "load_packed12_batch" if kind == "p12" else "load_packed16_batch"
        a = getattr(off, fn)([t, t, t], defects=[m, None, m])
        b = getattr(on, fn)([t, t, t], defects=[m, None, m])
        for x, y in zip(a, b):
            assert_exact(y.cpu().numpy(), x.cpu().numpy(), f"{cam} {fn} identity")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("radius", [1, 2])
def test_listed_defect_never_feeds_a_neighbour(ti, rng, dev, monkeypatch, cam, work, radius):
    """A listed site stuck at two values gives the same route CFA everywhere (its own output is the fix-up); without the
    map its neighbours differ."""
    H, W = 64, 128
    r, c = 30, 61
    codes = O.decode12(natural_packed12(rng, H, W, O.RGGB), "u16")
    base = codes[r, c]
    frames = {}
    for v in (min(int(base) + 40, 4095), max(int(base) - 40, 0)):
        codes[r, c] = v
        frames[v] = torch.from_numpy(O.encode12(codes)).to(dev)
    m = ti.DefectMap([[r, c]], (H, W))
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, raw_denoise=ti.RawDenoise(0.002, 0.01, radius=radius))
    got = capture(monkeypatch, isp)
    for f in frames.values():
        isp.load_packed12(f, defects=m)
    assert_exact(got[0].cpu().numpy(), got[1].cpu().numpy(), f"{cam} R={radius} with the map")
    for f in frames.values():
        isp.load_packed12(f)
    a, b = got[2].cpu().numpy(), got[3].cpu().numpy()
    near = np.zeros((H, W), bool)
    near[r - 2 * radius:r + 2 * radius + 1:2, c - 2 * radius:c + 2 * radius + 1:2] = True
    near[r, c] = False
    assert not np.array_equal(a[near], b[near]), "without the map the stuck value reaches its neighbours"


def test_process_packed12_matches_two_calls(ti, rng, dev):
    H, W = 64, 256
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(3)]
    a = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, raw_denoise=DN[1])
    b = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, raw_denoise=DN[1])
    for step in range(3):
        outs, imgs = a.process_packed12(frames, gamma=0.7, keep_images=True)
        ref_imgs = b.load_packed12_batch(frames)
        ref_outs = b.tonemap_reinhard(ref_imgs, gamma=0.7)
        for o, r in zip(outs, ref_outs):
            assert_exact(o.cpu().numpy(), r.cpu().numpy(), f"step {step} u8")
        for i, r in zip(imgs, ref_imgs):
            assert_exact(i.cpu().numpy(), r.cpu().numpy(), f"step {step} images")
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), f"step {step} metering state")


def test_set_turns_it_on_and_off(ti, rng, dev):
    H, W = 64, 256
    t = torch.from_numpy(natural_packed12(rng, H, W, O.RGGB)).to(dev)
    plain = ti.Camera32(ti.BayerPattern.RGGB, device=dev)
    isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev)
    want = plain.load_packed12(t).cpu().numpy()
    isp.set(raw_denoise=DN[1])
    assert isp.raw_denoise == DN[1]
    assert not np.array_equal(isp.load_packed12(t).cpu().numpy(), want)
    isp.set(moving_alpha=0.2)                                          # (None leaves it)
    assert isp.raw_denoise == DN[1]
    isp.set(raw_denoise=False)
    assert isp.raw_denoise is None
    assert_exact(isp.load_packed12(t).cpu().numpy(), want, "off again")
    with pytest.raises(ValueError):
        isp.set(raw_denoise=(0.1, 0.2))


@pytest.mark.parametrize("cam,work", CAMS)
def test_graph_capture_of_a_step(ti, rng, dev, cam, work):
    H, W = 64, 256
    frames = [[torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.02 * ((k + j) % 3))).to(dev)
               for j in range(2)] for k in range(4)]
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    static = [torch.empty_like(f) for f in frames[0]]
    kw = dict(moving_alpha=0.5, device=dev, raw_denoise=DN[2], lens_shading=make_grid(rng, 5, 5, 4))
    cap = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    eager = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)

    def step(isp, srcs):
        imgs = isp.load_packed12_batch(srcs, defects=[m, None])
        return imgs, isp.tonemap_reinhard(imgs, write_back=False)

    for s, f in zip(static, frames[0]):
        s.copy_(f)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step(cap, static)                                    # (warm-up: the first step, eagerly, on the capture stream)
    torch.cuda.current_stream(dev).wait_stream(side)
    step(eager, frames[0])
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        imgs, outs = step(cap, static)
    for k in range(1, 4):
        for s, f in zip(static, frames[k]):
            s.copy_(f)
        g.replay()
        want, want_outs = step(eager, frames[k])
        torch.cuda.synchronize(dev)
        for a, b in zip(imgs, want):
            assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"replay {k} images")
        if k == 1:                 # (a captured update_metering reads the metering state it was captured with)
            for a, b in zip(outs, want_outs):
                assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"replay {k} u8")


def test_batch_of_six_4k_cameras_equals_single_loads(ti, rng, dev):
    H, W = 3072, 4096
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.01 * k)).to(dev) for k in range(6)]
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, raw_denoise=DN[1], black_level=64)
    batch = isp.load_packed12_batch(frames)
    for k, f in enumerate(frames):
        assert torch.equal(batch[k], isp.load_packed12(f)), f"camera {k}"


def test_batch_beyond_one_launch(ti, rng, dev):
    """More frames than one launch takes (32): the second launch's frames as single loads."""
    H, W = 18, 36
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.005 * k)).to(dev) for k in range(35)]
    isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev, raw_denoise=DN[2])
    batch = isp.load_packed12_batch(frames)
    for k in (0, 31, 32, 34):
        assert torch.equal(batch[k], isp.load_packed12(frames[k])), f"frame {k}"
