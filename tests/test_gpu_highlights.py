"""Highlight reconstruction (Camera16/32 highlights=, reconstruct_cfa) on the GPU against tests/highlights_ref.py.

The route's CFA is captured by wrapping ISP._process_image; it must equal the NumPy f32 contract bit for bit (with the
defect fix-up of tests/test_defects_cpu.py at listed sites), and the loader's image must be O.bayer_to_rgb /
O.resize_bilinear of that CFA bit for bit.  The tile is 64 x 64: the shapes are the smallest that reach every seam."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import denoise_ref as D
from tests import highlights_ref as R
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_denoise import call, capture, loader_x
from tests.test_gpu_shading import PER_SITE, make_grid, pixel_gains
from tests.util import assert_exact

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
CCM = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
WB = np.array([1.8, 1.0, 2.1])
SHAPES = [(2, 2), (2, 4), (6, 4), (64, 64), (66, 70), (130, 66)]
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def source(rng, kind, H, W, pattern=O.RGGB, levels=False, clipped=True):
    """(the loader's input, x as the loader computes it, black, white, the clip level in x units) of a generated frame."""
    lv = levels and kind in ("p12", "ids", "p16", "16u")
    full = {"p12": 4095, "ids": 4095, "p16": 65535, "16u": 65535, "16f": 1000, "32f": 4095}[kind]
    black, white = (PER_SITE, full - 195) if lv else (None, None)
    clip = 980.0 if kind == "16f" else 0.98
    # the smallest code that every site calls clipped
    probe = np.repeat(np.arange(full + 1, dtype=np.uint16), 2)[None].repeat(2, 0)
    px = loader_x(kind, probe.astype(f32) * f32(1 / 4095) if kind == "32f" else probe, black, white)
    every = (px >= f32(clip)).reshape(2, full + 1, 2).all(axis=(0, 2))
    assert every.any()
    lo = int(np.argmax(every))
    codes = R.make_codes(rng, H, W, full, lo, pattern, clipped)
    if kind in ("p12", "ids"):
        src = O.encode12(codes, ids_format=kind == "ids")
        codes = O.decode12(src, "u16", ids_format=kind == "ids")          # (the IDS packing does not round-trip)
    elif kind == "p16":
        src = codes.view(np.uint8).reshape(H, 2 * W)
    elif kind == "32f":
        src = codes = codes.astype(f32) * f32(1 / 4095)
    else:
        src = codes
    return src, loader_x(kind, codes, black, white), black, white, clip


def assert_exercised(x, y, clip, what):
    """On the reference alone: a frame of 4096 pixels or more has 5 % of its pixels raised and, per site, a clipped pixel
    that is left unchanged."""
    H, W = x.shape
    if H * W >= 4096:
        frac, kept = R.coverage(x, y, clip, H, W)
        assert frac >= 0.05 and min(kept) >= 1, f"{what}: the frame does not exercise the operator ({frac}, {kept})"


def balance_of(isp):
    """The balance gains the route uses, read back from the ISP."""
    if isp.auto_white_balance is not None:
        return isp._awb_gains.cpu().numpy()
    return np.asarray(isp.white_balance, f32) if isp.correct_colors else np.ones(3, f32)


def expected_cfa(isp, x, pattern, work, mask=None):
    """(the route's CFA with the fix-up, y) from the reference."""
    H, W = x.shape
    hl = isp.highlights
    grid = isp._applied_shading()
    gain = None if grid is None else pixel_gains(grid.cpu().numpy(), H, W)
    y = R.reconstruct(x, pattern, balance_of(isp), hl.mode, hl.clip, mask)
    cfa = O.cast_out(y if gain is None else (y * gain).astype(f32), work)
    return (cfa if mask is None else correct_cfa(cfa, mask, work)), y


def check_image(isp, img, cfa, pattern, what):
    H, W = cfa.shape
    rgb = O.bayer_to_rgb(cfa, pattern, correct_colors=isp.color_correct_matrix)
    sz = O.isp_output_size(H, W, isp.resize_width, None)
    assert_exact(img, rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1]), what + " image")


# ---- reconstruct_cfa ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("mode", ["rebuild", "clip"])
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
def test_reconstruct_cfa(ti, rng, dev, work, mode, pattern):
    for H, W in SHAPES + [(1, 5), (3, 1), (65, 67)]:
        codes = R.make_codes(rng, H, W, 4095, int(0.985 * 4095) + 1, pattern)
        x = O.cast_out(codes.astype(f32) * f32(1 / 4095), work)
        hl = ti.Highlights(mode, 0.98)
        want = O.cast_out(R.reconstruct(x.astype(f32), pattern, f32(WB), mode, 0.98), work)
        if mode == "rebuild":
            assert_exercised(x.astype(f32), R.reconstruct(x.astype(f32), pattern, f32(WB)), 0.98, f"{H}x{W}")
        got = ti.highlights.reconstruct_cfa(torch.from_numpy(x).to(dev), ti.BayerPattern(pattern), WB, hl)
        assert got.device == dev and got.shape == (H, W)
        assert_exact(got.cpu().numpy(), want, f"{work} {mode} p{pattern} {H}x{W}")
        host = ti.highlights.reconstruct_cfa(x, ti.BayerPattern(pattern), tuple(WB), hl)     # numpy in, numpy out
        assert isinstance(host, np.ndarray)
        assert_exact(host, want, "numpy round trip")
    empty = ti.highlights.reconstruct_cfa(np.zeros((0, 8), f32), ti.BayerPattern.RGGB)
    assert empty.shape == (0, 8)


def test_reconstruct_cfa_defaults_and_identity(ti, rng, dev):
    x = (rng.random((66, 70)) * 0.97).astype(f32)
    assert_exact(ti.highlights.reconstruct_cfa(x, ti.BayerPattern.GRBG, WB), x, "no clipped pixel")
    x[10:20, 30:50] = 1.0
    want = R.reconstruct(x, O.GRBG, (1, 1, 1))                                  # (the default balance and settings)
    assert_exact(ti.highlights.reconstruct_cfa(x, ti.BayerPattern.GRBG), want, "defaults")
    # pixels exactly at t are clipped (>=): t = 0.75 is exact in f16 and f32
    for work in ("f16", "f32"):
        x = O.cast_out(np.full((66, 70), 0.625, f32), work)
        x[::3, ::5] = 0.75
        want = R.reconstruct(x.astype(f32), O.GRBG, f32(WB), "rebuild", 0.75)
        assert (want[::3, ::5] > 0.75).sum() > 50, "the pixels at t must be raised for the case to show anything"
        got = ti.highlights.reconstruct_cfa(x, ti.BayerPattern.GRBG, WB, ti.Highlights("rebuild", 0.75))
        assert_exact(got, O.cast_out(want, work), f"{work} x == t")


# ---- the loaders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["rebuild", "clip"])
def test_every_source_kind_and_shape(ti, rng, dev, monkeypatch, cam, work, kind, mode):
    """Every source kind, both work dtypes and modes at every shape; levels and a per-site grid at the seam shapes."""
    for i, (H, W) in enumerate(SHAPES):
        pattern = i % 4
        extras = H * W >= 4096 and (i & 1) == 0
        src, x, black, white, clip = source(rng, kind, H, W, pattern, levels=extras)
        grid = make_grid(rng, 5, 7, 4) if extras else None
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, color_correction=CCM,
                               black_level=black, white_level=white, lens_shading=grid,
                               highlights=ti.Highlights(mode, clip))
        got = capture(monkeypatch, isp)
        img = call(isp, kind, torch.from_numpy(src).to(dev)).cpu().numpy()
        want, y = expected_cfa(isp, x, pattern, work)
        what = f"{cam} {kind} {mode} p{pattern} {H}x{W} extras={extras}"
        if mode == "rebuild":
            assert_exercised(x, y, clip, what)
        assert_exact(got[0].cpu().numpy(), want, what + " CFA")
        check_image(isp, img, want, pattern, what)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", ["rebuild", "clip"])
def test_patterns_with_a_defect_map(ti, rng, dev, monkeypatch, cam, work, pattern, mode):
    """The four patterns with a defect map whose entries sit next to, and on, clipped pixels (and the map of the defect
    tests: borders, corners, clusters); without correct_colors the balance is (1, 1, 1)."""
    H, W = 66, 70
    for correct in (True, False):
        src, x, black, white, clip = source(rng, "p12", H, W, pattern)
        clipped = np.argwhere(x >= f32(clip))
        pick = clipped[:: max(1, len(clipped) // 12)]
        sites = {(int(r), int(c)) for r, c in pick}                                       # on clipped pixels ...
        sites |= {(int(r), int(c) + 1) for r, c in pick[::2] if c + 1 < W}                # ... and next to them
        sites |= {(int(r) + 1, int(c)) for r, c in pick[1::2] if r + 1 < H}
        sites |= {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (63, 63), (64, 64), (63, 64), (1, 1)}
        m = ti.DefectMap(sorted(sites), (H, W))
        mask = m.mask()
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=correct,
                               highlights=ti.Highlights(mode, clip), lens_shading=make_grid(rng, 3, 4, 1))
        got = capture(monkeypatch, isp)
        img = isp.load_packed12(torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
        want, y = expected_cfa(isp, x, pattern, work, mask)
        what = f"{cam} p{pattern} {mode} correct_colors={correct}"
        if mode == "rebuild":
            assert_exercised(x, y, clip, what)
            y_nomap = R.reconstruct(x, pattern, balance_of(isp), mode, clip)
            assert not np.array_equal(y, y_nomap), "the map changes no estimate: the case shows nothing"
        assert_exact(got[0].cpu().numpy(), want, what + " CFA")
        check_image(isp, img, want, pattern, what)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_awb_gains_after_an_update(ti, rng, dev, monkeypatch, cam, work, kind):
    """AWB on: the balance gains are the device's current ones (read back for the reference), the grid is E."""
    H, W = 66, 70
    pattern = O.GBRG
    src, x, black, white, clip = source(rng, kind, H, W, pattern, levels=True)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, black_level=black, white_level=white,
                           auto_white_balance=True, moving_alpha=0.5, highlights=ti.Highlights("rebuild", clip))
    t = torch.from_numpy(src).to(dev)
    isp.tonemap_reinhard([call(isp, kind, t)])                                # (one update of the gains)
    gains = isp._awb_gains.cpu().numpy()
    assert not np.array_equal(gains, f32(WB)), "the update left the seed"
    got = capture(monkeypatch, isp)
    img = call(isp, kind, t).cpu().numpy()
    want, y = expected_cfa(isp, x, pattern, work)
    assert_exercised(x, y, clip, f"{cam} {kind} awb")
    assert_exact(got[0].cpu().numpy(), want, f"{cam} {kind} awb CFA")
    check_image(isp, img, want, pattern, f"{cam} {kind} awb")


@pytest.mark.parametrize("cam,work", CAMS)
def test_reference_quirks_resize_and_lens(ti, rng, dev, monkeypatch, cam, work):
    H, W = 66, 70
    src, x, black, white, clip = source(rng, "p12", H, W, O.RGGB)
    t = torch.from_numpy(src).to(dev)
    # reference_quirks: the demosaic, and so the sites' colours, are RGGB whatever bayer_pattern says
    isp = getattr(ti, cam)(ti.BayerPattern.GRBG, device=dev, correct_colors=True, reference_quirks=True,
                           resize_width=36, highlights=ti.Highlights("rebuild", clip))
    got = capture(monkeypatch, isp)
    img = isp.load_packed12(t).cpu().numpy()
    want, y = expected_cfa(isp, x, O.RGGB, work)
    assert_exercised(x, y, clip, "quirks")
    assert not np.array_equal(y, R.reconstruct(x, O.GRBG, f32(WB), "rebuild", clip))
    assert_exact(got[0].cpu().numpy(), want, f"{cam} reference_quirks CFA")
    check_image(isp, img, want, O.RGGB, f"{cam} reference_quirks resize_width=36")
    # a lens: the image is the remap of the demosaiced route CFA, as a plain ISP gives it from the reference's y
    K = np.array([[60.0, 0, W / 2 - 3], [0, 62.0, H / 2 + 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, (-0.2, 0.05, 0.001, -0.002), (H, W))
    kw = dict(device=dev, correct_colors=True, scale=0.5)
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, highlights=ti.Highlights("rebuild", clip), **kw)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    got.clear()
    img = isp.load_packed12(t, undistort=lens).cpu().numpy()
    want, y = expected_cfa(isp, x, O.RGGB, work)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} lens CFA")
    assert_exact(img, plain.load_32f(torch.from_numpy(y).to(dev), undistort=lens).cpu().numpy(), f"{cam} lens image")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("bits", [12, 16])
def test_batch_forms(ti, rng, dev, monkeypatch, cam, work, bits):
    H, W = 66, 70
    kind = "p12" if bits == 12 else "p16"
    srcs = [source(rng, kind, H, W, O.BGGR, levels=True) for _ in range(3)]
    black, white, clip = srcs[0][2:]
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64), (65, 69)], (H, W))
    isp = getattr(ti, cam)(ti.BayerPattern.BGGR, device=dev, correct_colors=True, black_level=black, white_level=white,
                           highlights=ti.Highlights("rebuild", clip), resize_width=36)
    got = capture(monkeypatch, isp)
    ts = [torch.from_numpy(s[0]).to(dev) for s in srcs]
    fn = isp.load_packed12_batch if bits == 12 else isp.load_packed16_batch
    imgs = fn(ts, defects=[m, None, m])
    for k, (s, im) in enumerate(zip(srcs, imgs)):
        want, y = expected_cfa(isp, s[1], O.BGGR, work, m.mask() if k != 1 else None)
        assert_exercised(s[1], y, clip, f"batch frame {k}")
        assert_exact(got[k].cpu().numpy(), want, f"{cam} {kind} batch frame {k} CFA")
        check_image(isp, im.cpu().numpy(), want, O.BGGR, f"{cam} {kind} batch frame {k}")
    # more frames than one launch takes (32): the second launch's frames as single loads
    small = [torch.from_numpy(source(rng, kind, 6, 4, O.BGGR, levels=True)[0]).to(dev) for _ in range(34)]
    batch = fn(small)
    for k in (0, 31, 32, 33):
        single = isp.load_packed12(small[k]) if bits == 12 else isp.load_packed16(small[k])
        assert torch.equal(batch[k], single), f"frame {k}"


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_no_clipped_pixel_and_set_off_are_bit_exact(ti, rng, dev, cam, work, kind):
    """A frame without a clipped pixel, and any frame after set(highlights=False), give the bits of an ISP that never had
    highlights - images and metering - with levels, shading, defects and the resize."""
    H, W = 66, 70
    src, x, black, white, clip = source(rng, kind, H, W, O.GBRG, levels=True, clipped=False)
    assert not (x >= f32(clip)).any()
    hot, *_ = source(rng, kind, H, W, O.GBRG, levels=True)
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64), (65, 69)], (H, W))
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white,
              lens_shading=make_grid(rng, 5, 7, 4), resize_width=36)
    off = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw)
    on = getattr(ti, cam)(ti.BayerPattern.GBRG, highlights=ti.Highlights("rebuild", clip), **kw)
    t, th = torch.from_numpy(src).to(dev), torch.from_numpy(hot).to(dev)
    a, b = call(off, kind, t, defects=m), call(on, kind, t, defects=m)
    assert_exact(b.cpu().numpy(), a.cpu().numpy(), f"{cam} {kind} no clipped pixel")
    off.tonemap_reinhard([a], gamma=0.9)
    on.tonemap_reinhard([b], gamma=0.9)
    assert_exact(on.metrics.cpu().numpy(), off.metrics.cpu().numpy(), "metering")
    assert not torch.equal(call(on, kind, th), call(off, kind, th)), "a clipped frame must differ"
    assert on.highlights == ti.Highlights("rebuild", clip)
    on.set(moving_alpha=0.2)                                                  # (None leaves it)
    assert on.highlights is not None
    on.set(highlights=ti.Highlights("clip", clip))
    assert on.highlights.mode == "clip"
    on.set(highlights=False)
    assert on.highlights is None
    assert_exact(call(on, kind, th, defects=m).cpu().numpy(), call(off, kind, th, defects=m).cpu().numpy(),
                 f"{cam} {kind} off again")
    with pytest.raises(ValueError):
        on.set(highlights="rebuild")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "p16", "16u", "32f"])
def test_composition_with_raw_denoise(ti, rng, dev, monkeypatch, cam, work, kind):
    """With raw noise reduction on as well: the highlights launch writes the plain f32 y (bit-exact against the
    reference), the filter runs on it with the same grid and maps, and the final CFA holds the filter's bound against
    the reference chain."""
    from tests.util import _count_calls
    H, W = 66, 70
    pattern = O.GRBG
    src, x, black, white, clip = source(rng, kind, H, W, pattern, levels=True)
    dn = ti.RawDenoise(0.002, 0.01, strength=1.5, radius=1)
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64), (65, 69), (33, 0)], (H, W))
    mask = m.mask()
    grid = make_grid(rng, 5, 7, 4)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, black_level=black, white_level=white,
                           lens_shading=grid, raw_denoise=dn, highlights=ti.Highlights("rebuild", clip))
    # the f32 y itself, through the C entry point the route calls
    from taichi_image_amd import _native
    t = torch.from_numpy(src).to(dev)
    ys = torch.empty((H, W), dtype=torch.float32, device=dev)
    raw_kind = {"p12": _native.MI_RAW_PACKED12, "p16": _native.MI_RAW_PACKED16, "16u": _native.MI_RAW_16U,
                "32f": _native.MI_RAW_32F}[kind]
    bits = {"p12": 12, "p16": 16}.get(kind, 16)
    lv = isp._levels(bits) if kind != "32f" else None
    arg = m._arg(dev)
    _native.check(_native.lib().mi_isp_highlights_raw(
        t.data_ptr(), ys.data_ptr(), H, W, raw_kind, 0, isp.dtype.code, pattern, lv, None, arg, isp._highlights_arg(), 1,
        _native.stream_ptr(dev)))
    y = R.reconstruct(x, pattern, f32(WB), "rebuild", clip, mask)
    assert_exercised(x, y, clip, f"{cam} {kind} composition")
    assert_exact(ys.cpu().numpy(), y, f"{cam} {kind} plain f32 y")
    # the route: one highlights launch, one denoise launch, the fix-up
    n_hl = _count_calls(monkeypatch, "mi_isp_highlights_raw_batch")
    n_dn = _count_calls(monkeypatch, "mi_isp_denoise_raw_batch")
    got = capture(monkeypatch, isp)
    img = call(isp, kind, t, defects=m).cpu().numpy()
    assert len(n_hl) == 1 and len(n_dn) == 1
    cfa = got[0].cpu().numpy()
    gain = pixel_gains(grid, H, W)
    D.assert_within_bound(cfa, D.route_yg(y, dn, gain, mask), work, f"{cam} {kind} chain", where=~mask)
    assert_exact(cfa, correct_cfa(cfa, mask, work), "defect fix-up")
    check_image(isp, img, cfa, pattern, f"{cam} {kind} chain")


def test_process_packed12_takes_the_two_calls(ti, rng, dev):
    H, W = 64, 64
    frames = [torch.from_numpy(source(rng, "p12", H, W)[0]).to(dev) for _ in range(3)]
    hl = ti.Highlights("rebuild", 0.98)
    a = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True, highlights=hl)
    b = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True, highlights=hl)
    for step in range(2):
        outs, imgs = a.process_packed12(frames, gamma=0.7, keep_images=True)
        ref_imgs = b.load_packed12_batch(frames)
        ref_outs = b.tonemap_reinhard(ref_imgs, gamma=0.7)
        for o, r in zip(outs, ref_outs):
            assert_exact(o.cpu().numpy(), r.cpu().numpy(), f"step {step} u8")
        for i, r in zip(imgs, ref_imgs):
            assert_exact(i.cpu().numpy(), r.cpu().numpy(), f"step {step} images")
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), f"step {step} metering state")


@pytest.mark.parametrize("cam,work", CAMS)
def test_graph_capture_of_a_step(ti, rng, dev, cam, work):
    """A load + tonemap step with highlights (AWB on: the gains are read on the device) is graph-capturable."""
    H, W = 66, 70
    frames = [[torch.from_numpy(source(rng, "p12", H, W)[0]).to(dev) for _ in range(2)] for _ in range(3)]
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64)], (H, W))
    static = [torch.empty_like(f) for f in frames[0]]
    kw = dict(moving_alpha=0.5, device=dev, correct_colors=True, auto_white_balance=True,
              highlights=ti.Highlights("rebuild", 0.98))
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
    for k in range(1, 3):
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
