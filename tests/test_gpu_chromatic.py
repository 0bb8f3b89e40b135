"""Chromatic aberration correction (Camera16/32 chromatic_aberration=, correct_cfa) on the GPU against
tests/chromatic_ref.py.

The route's CFA is captured by wrapping ISP._process_image; it must equal the NumPy f32 contract bit for bit (with the
defect fix-up of tests/test_defects_cpu.py at listed sites), and the loader's image must be O.bayer_to_rgb /
O.resize_bilinear of that CFA bit for bit.  The tile is 64 x 64 and the shift reaches 5.8 px: the shapes are the smallest
that reach every seam with a shift that crosses it."""
import math

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chromatic_ref as R
from tests import denoise_ref as D
from tests import highlights_ref as HR
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_denoise import call, capture, loader_x
from tests.test_gpu_shading import PER_SITE, make_grid, pixel_gains
from tests.util import _count_calls, assert_exact

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
CCM = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
WB = np.array([1.8, 1.0, 2.1])
SHAPES = [(2, 2), (2, 4), (6, 4), (64, 64), (66, 70), (130, 66)]
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]
ENTRIES = ["mi_isp_chromatic_raw", "mi_isp_chromatic_raw_batch", "mi_isp_chromatic_cfa"]
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def settings(ti, H, W, **kw):
    k = R.frame_settings(H, W)
    return ti.ChromaticAberration(k.red, k.blue, **kw)


def source(rng, kind, H, W, levels=False):
    """(the loader's input, x as the loader computes it, black, white) of a frame of random codes."""
    lv = levels and kind in ("p12", "ids", "p16", "16u")
    full = {"p12": 4095, "ids": 4095, "p16": 65535, "16u": 65535, "16f": 16000, "32f": 4095}[kind]   # (16f: f16 images hold the values)
    black, white = (PER_SITE, full - 195) if lv else (None, None)
    codes = rng.integers(0, full + 1, (H, W)).astype(np.uint16)
    if kind in ("p12", "ids"):
        src = O.encode12(codes, ids_format=kind == "ids")
        codes = O.decode12(src, "u16", ids_format=kind == "ids")          # (the IDS packing does not round-trip)
    elif kind == "p16":
        src = codes.view(np.uint8).reshape(H, 2 * W)
    elif kind == "32f":
        src = codes = codes.astype(f32) * f32(1 / 4095)
    else:
        src = codes
    return src, loader_x(kind, codes, black, white), black, white


def assert_exercised(x, pattern, ca, what):
    """On the reference alone: on a frame of 4096 pixels or more, half of the red / blue pixels sample another cell, 4 %
    have a clamped tap and every pixel that can change does (tests/test_chromatic_cpu.py)."""
    if x.size >= 4096:
        moved, clamped, changed, fixed = R.coverage(x, pattern, ca)
        assert moved >= 0.5 and clamped >= 0.04 and changed == 1.0 and fixed < 0.005, \
            f"{what}: the frame does not exercise the operator ({moved}, {clamped}, {changed}, {fixed})"


def expected_cfa(isp, x, pattern, work, mask=None, y=None):
    """(the route's CFA with the fix-up, y) from the reference; y given: the stage's output from elsewhere."""
    H, W = x.shape
    grid = isp._applied_shading()
    gain = None if grid is None else pixel_gains(grid.cpu().numpy(), H, W)
    if y is None:
        y = R.correct(x, pattern, isp.chromatic_aberration, mask)
    cfa = O.cast_out(y if gain is None else (y * gain).astype(f32), work)
    return (cfa if mask is None else correct_cfa(cfa, mask, work)), y


def check_image(isp, img, cfa, pattern, what):
    H, W = cfa.shape
    rgb = O.bayer_to_rgb(cfa, pattern, correct_colors=isp.color_correct_matrix)
    sz = O.isp_output_size(H, W, isp.resize_width, None)
    assert_exact(img, rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1]), what + " image")


def seam_defects(ti, rng, H, W):
    """A defect map whose sites sit among the taps of pixels on both sides of the tile seams (rows / columns 52 .. 75: the
    shift reaches 5.8 px), at the frame's corners and scattered over the frame, clusters of same-colour neighbours
    included."""
    sites = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (1, 1), (H - 2, W - 2)}
    for r in range(max(0, min(52, H - 14)), min(H, 76)):
        for c in range(max(0, min(52, W - 18)), min(W, 76)):
            if rng.random() < 0.12:
                sites.add((r, c))
    for r, c in [(58, 60), (62, 62), (64, 64), (66, 60), (20, 62), (62, 20)]:
        if r + 2 < H and c + 2 < W:
            sites |= {(r, c), (r, c + 2), (r + 2, c), (r + 2, c + 2)}        # four taps of one colour: all masked
    sites |= {(int(r), int(c)) for r, c in zip(rng.integers(0, H, 40), rng.integers(0, W, 40))}
    return ti.DefectMap(sorted(sites), (H, W))


# ---- correct_cfa ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
def test_correct_cfa(ti, rng, dev, work, pattern):
    for H, W in SHAPES + [(1, 5), (3, 1), (65, 67)]:
        x = O.cast_out(rng.random((H, W)).astype(f32), work)
        ca = settings(ti, H, W)
        want = O.cast_out(R.correct(x.astype(f32), pattern, ca), work)
        assert_exercised(x.astype(f32), pattern, ca, f"{H}x{W}")
        got = ti.chromatic.correct_cfa(torch.from_numpy(x).to(dev), ti.BayerPattern(pattern), ca)
        assert got.device == dev and got.shape == (H, W)
        assert_exact(got.cpu().numpy(), want, f"{work} p{pattern} {H}x{W}")
        host = ti.chromatic.correct_cfa(x, ti.BayerPattern(pattern), ca)        # numpy in, numpy out
        assert isinstance(host, np.ndarray)
        assert_exact(host, want, "numpy round trip")
    empty = ti.chromatic.correct_cfa(np.zeros((0, 8), f32), ti.BayerPattern.RGGB, ti.ChromaticAberration())
    assert empty.shape == (0, 8)


def test_correct_cfa_identity_center_and_norm_radius(ti, rng, dev):
    x = rng.random((66, 70)).astype(f32)
    ident = ti.ChromaticAberration(center=(20.3, 41.77), norm_radius=37.5)
    assert_exact(ti.chromatic.correct_cfa(x, ti.BayerPattern.GRBG, ident), x, "identity coefficients")
    # a centre off the middle (and off the frame's half-integer grid), a radius of its own; the largest shift is at the
    # corner farthest from the centre: 6.9 px (red), 5.6 px (blue)
    for H, W, center, nr in [(66, 70, (20.3, 41.77), 60.0), (130, 66, (-3.5, 70.25), 150.0), (65, 67, (32.0, 33.0), 40.0)]:
        far = math.hypot(max(abs(center[0]), abs(H - 1 - center[0])), max(abs(center[1]), abs(W - 1 - center[1])))
        q = (far / nr) ** 2
        ca = ti.ChromaticAberration((1 + 3 / far, 2 / far / q, 1.9 / far / q / q), (1 - 2 / far, -2.5 / far / q, -1.1 / far / q / q),
                                    center=center, norm_radius=nr)
        assert 6.5 < ca.max_shift((H, W))[0] <= 8 and 5 < ca.max_shift((H, W))[1] <= 8
        x = rng.random((H, W)).astype(f32)
        for pattern in (O.RGGB, O.GBRG):
            want = R.correct(x, pattern, ca)
            assert not np.array_equal(want, R.correct(x, pattern, ti.ChromaticAberration(ca.red, ca.blue)))
            got = ti.chromatic.correct_cfa(x, ti.BayerPattern(pattern), ca)
            assert_exact(got, want, f"{H}x{W} centre {center} norm_radius {nr} p{pattern}")


# ---- the loaders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_source_kind_and_shape(ti, rng, dev, monkeypatch, cam, work, kind):
    """Every source kind and both work dtypes at every shape; levels and a per-site grid at the seam shapes."""
    for i, (H, W) in enumerate(SHAPES):
        pattern = i % 4
        extras = H * W >= 4096 and (i & 1) == 0
        src, x, black, white = source(rng, kind, H, W, levels=extras)
        grid = make_grid(rng, 5, 7, 4) if extras else None
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, color_correction=CCM,
                               black_level=black, white_level=white, lens_shading=grid,
                               chromatic_aberration=settings(ti, H, W))
        got = capture(monkeypatch, isp)
        img = call(isp, kind, torch.from_numpy(src).to(dev)).cpu().numpy()
        want, y = expected_cfa(isp, x, pattern, work)
        what = f"{cam} {kind} p{pattern} {H}x{W} extras={extras}"
        assert_exercised(x, pattern, isp.chromatic_aberration, what)
        assert_exact(got[0].cpu().numpy(), want, what + " CFA")
        assert_exact(want, R.route_cfa(x, pattern, isp.chromatic_aberration, work,
                                       None if grid is None else pixel_gains(grid, H, W)), "route_cfa")
        check_image(isp, img, want, pattern, what)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
def test_patterns_with_a_defect_map(ti, rng, dev, monkeypatch, cam, work, pattern):
    """The four patterns with a defect map whose sites sit among the taps on both sides of the tile seams; a non-default
    centre and norm_radius on the second shape."""
    for H, W, kw in [(66, 70, {}), (130, 66, dict(center=(70.2, 30.9), norm_radius=95.0))]:
        src, x, black, white = source(rng, "p12", H, W)
        m = seam_defects(ti, rng, H, W)
        mask = m.mask()
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, lens_shading=make_grid(rng, 3, 4, 1),
                               chromatic_aberration=settings(ti, H, W, **kw))
        got = capture(monkeypatch, isp)
        img = isp.load_packed12(torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
        want, y = expected_cfa(isp, x, pattern, work, mask)
        y_nomap = R.correct(x, pattern, isp.chromatic_aberration)
        changed = (y != y_nomap) & ~mask
        assert changed.sum() >= 50, "the map changes too few estimates: the case shows nothing"
        for part in (changed[:64], changed[64:], changed[:, :64], changed[:, 64:]):   # ... on both sides of the seams
            assert part.any(), "the map feeds no tap on one side of a seam"
        what = f"{cam} p{pattern} {H}x{W} defects"
        assert_exact(got[0].cpu().numpy(), want, what + " CFA")
        check_image(isp, img, want, pattern, what)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_awb_grid_and_statistics(ti, rng, dev, monkeypatch, cam, work, kind):
    """AWB on: the effective grid E is the gain the stage applies, and the statistics (which read the source) are those of
    an ISP without the stage."""
    H, W = 66, 70
    pattern = O.GBRG
    src, x, black, white = source(rng, kind, H, W, levels=True)
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white, auto_white_balance=True,
              moving_alpha=0.5, lens_shading=make_grid(rng, 5, 7, 4))
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), chromatic_aberration=settings(ti, H, W), **kw)
    plain = getattr(ti, cam)(ti.BayerPattern(pattern), **kw)
    t = torch.from_numpy(src).to(dev)
    call(isp, kind, t)
    call(plain, kind, t)
    assert_exact(isp._awb_pending.cpu().numpy(), plain._awb_pending.cpu().numpy(), "pending statistics")
    isp.update_white_balance()
    plain.update_white_balance()
    assert_exact(isp._awb_gains.cpu().numpy(), plain._awb_gains.cpu().numpy(), "gains after an update")
    assert not np.array_equal(isp._awb_gains.cpu().numpy(), f32(WB)), "the update left the seed"
    got = capture(monkeypatch, isp)
    img = call(isp, kind, t).cpu().numpy()
    want, y = expected_cfa(isp, x, pattern, work)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} {kind} awb CFA")
    check_image(isp, img, want, pattern, f"{cam} {kind} awb")


@pytest.mark.parametrize("cam,work", CAMS)
def test_reference_quirks_resize_and_lens(ti, rng, dev, monkeypatch, cam, work):
    H, W = 66, 70
    src, x, black, white = source(rng, "p12", H, W)
    t = torch.from_numpy(src).to(dev)
    ca = settings(ti, H, W)
    # reference_quirks: the demosaic, and so the sites' colours, are RGGB whatever bayer_pattern says
    isp = getattr(ti, cam)(ti.BayerPattern.GRBG, device=dev, correct_colors=True, reference_quirks=True,
                           resize_width=36, chromatic_aberration=ca)
    got = capture(monkeypatch, isp)
    img = isp.load_packed12(t).cpu().numpy()
    want, y = expected_cfa(isp, x, O.RGGB, work)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} reference_quirks CFA")
    check_image(isp, img, want, O.RGGB, f"{cam} reference_quirks resize_width=36")
    # a lens: the per-frame remap still follows: the image is the remap of the demosaiced route CFA
    K = np.array([[60.0, 0, W / 2 - 3], [0, 62.0, H / 2 + 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, (-0.2, 0.05, 0.001, -0.002), (H, W))
    kw = dict(device=dev, correct_colors=True, scale=0.5)
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, chromatic_aberration=ca, **kw)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    got.clear()
    img = isp.load_packed12(t, undistort=lens).cpu().numpy()
    want, y = expected_cfa(isp, x, O.RGGB, work)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} lens CFA")
    assert_exact(img, plain.load_32f(torch.from_numpy(y).to(dev), undistort=lens).cpu().numpy(), f"{cam} lens image")


# ---- chains ------------------------------------------------------------------------------------------------------------
def clipped_source(rng, kind, H, W, pattern):
    """A frame with clipped blobs (tests/highlights_ref.make_codes) for the chains that start with highlights."""
    full = {"p12": 4095, "16u": 65535}[kind]
    codes = HR.make_codes(rng, H, W, full, int(0.985 * full) + 1, pattern)
    src = O.encode12(codes) if kind == "p12" else codes
    return src, loader_x(kind, codes, None, None)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_chain_highlights_then_chromatic(ti, rng, dev, monkeypatch, cam, work, kind):
    """Highlights -> chromatic aberration: the NumPy stages composed in that order, bit for bit, one launch each."""
    H, W = 66, 70
    pattern = O.GRBG
    src, x = clipped_source(rng, kind, H, W, pattern)
    m = seam_defects(ti, rng, H, W)
    mask = m.mask()
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, lens_shading=make_grid(rng, 5, 7, 4),
                           highlights=ti.Highlights("rebuild", 0.98), chromatic_aberration=settings(ti, H, W))
    n_hl = _count_calls(monkeypatch, "mi_isp_highlights_raw_batch")
    n_ca = _count_calls(monkeypatch, "mi_isp_chromatic_raw_batch")
    n_dn = _count_calls(monkeypatch, "mi_isp_denoise_raw_batch")
    got = capture(monkeypatch, isp)
    img = call(isp, kind, torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
    assert (len(n_hl), len(n_ca), len(n_dn)) == (1, 1, 0)
    y_hl = HR.reconstruct(x, pattern, f32(WB), "rebuild", 0.98, mask)
    assert (y_hl > x).mean() >= 0.05, "the frame has too few rebuilt pixels"
    y = R.correct(y_hl, pattern, isp.chromatic_aberration, mask)
    assert not np.array_equal(y, R.correct(x, pattern, isp.chromatic_aberration, mask))
    want, _ = expected_cfa(isp, x, pattern, work, mask, y=y)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} {kind} highlights -> chromatic CFA")
    check_image(isp, img, want, pattern, f"{cam} {kind} highlights -> chromatic")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
@pytest.mark.parametrize("with_highlights", [False, True])
def test_chains_that_end_in_raw_denoise(ti, rng, dev, monkeypatch, cam, work, kind, with_highlights):
    """Chromatic aberration -> raw denoise, and all three stages: the stage's plain f32 y is bit-exact (through the C entry
    point the route calls), and the final CFA holds the filter's bound against the NumPy chain."""
    from taichi_image_amd import _native
    H, W = 66, 70
    pattern = O.GRBG
    src, x = clipped_source(rng, kind, H, W, pattern)
    dn = ti.RawDenoise(0.002, 0.01, strength=1.5, radius=1)
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64), (65, 69), (33, 0), (60, 62), (62, 66), (66 - 2, 58)], (H, W))
    mask = m.mask()
    grid = make_grid(rng, 5, 7, 4)
    hl = ti.Highlights("rebuild", 0.98) if with_highlights else None
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, lens_shading=grid, raw_denoise=dn,
                           highlights=hl, chromatic_aberration=settings(ti, H, W))
    y0 = HR.reconstruct(x, pattern, f32(WB), "rebuild", 0.98, mask) if with_highlights else x
    y = R.correct(y0, pattern, isp.chromatic_aberration, mask)
    # the stage's plain f32 y from the f32 values in front of it
    t0 = torch.from_numpy(y0).to(dev)
    ys = torch.empty((H, W), dtype=torch.float32, device=dev)
    arg = m._arg(dev)
    _native.check(_native.lib().mi_isp_chromatic_raw(
        t0.data_ptr(), ys.data_ptr(), H, W, _native.MI_RAW_32F, 0, isp.dtype.code, pattern, None, None, arg,
        isp.chromatic_aberration._arg((H, W)), 1, _native.stream_ptr(dev)))
    assert_exact(ys.cpu().numpy(), y, f"{cam} {kind} plain f32 y")
    n_hl = _count_calls(monkeypatch, "mi_isp_highlights_raw_batch")
    n_ca = _count_calls(monkeypatch, "mi_isp_chromatic_raw_batch")
    n_dn = _count_calls(monkeypatch, "mi_isp_denoise_raw_batch")
    got = capture(monkeypatch, isp)
    img = call(isp, kind, torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
    assert (len(n_hl), len(n_ca), len(n_dn)) == (int(with_highlights), 1, 1)
    cfa = got[0].cpu().numpy()
    D.assert_within_bound(cfa, D.route_yg(y, dn, pixel_gains(grid, H, W), mask), work, f"{cam} {kind} chain", where=~mask)
    assert_exact(cfa, correct_cfa(cfa, mask, work), "defect fix-up")
    check_image(isp, img, cfa, pattern, f"{cam} {kind} chain")


# ---- on, off, limits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_set_and_unchanged_behaviour_when_off(ti, rng, dev, monkeypatch, cam, work, kind):
    """An ISP without the stage, and one after set(chromatic_aberration=False), call no mi_isp_chromatic_* entry point and
    give the bits of the plain loaders - images and metering - with levels, shading, defects and the resize."""
    H, W = 66, 70
    src, x, black, white = source(rng, kind, H, W, levels=True)
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64), (65, 69)], (H, W))
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white,
              lens_shading=make_grid(rng, 5, 7, 4), resize_width=36)
    ca = settings(ti, H, W)
    off = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw)
    on = getattr(ti, cam)(ti.BayerPattern.GBRG, chromatic_aberration=ca, **kw)
    assert off.chromatic_aberration is None and on.chromatic_aberration == ca
    t = torch.from_numpy(src).to(dev)
    calls = [_count_calls(monkeypatch, e) for e in ENTRIES]
    a = call(off, kind, t, defects=m)
    assert sum(len(c) for c in calls) == 0, "an ISP without the stage reached a chromatic entry point"
    # the plain loaders' contract: cast(x * g), the fix-up, the demosaic and the resize of the oracle
    gain = pixel_gains(off._applied_shading().cpu().numpy(), H, W)
    check_image(off, a.cpu().numpy(), correct_cfa(O.cast_out((x * gain).astype(f32), work), m.mask(), work), O.GBRG, "off")
    b = call(on, kind, t, defects=m)
    assert sum(len(c) for c in calls) == 1
    assert not torch.equal(a, b), "the stage must change a random frame"
    on.set(moving_alpha=0.2)                                                  # (None leaves it)
    assert on.chromatic_aberration == ca
    other = ti.ChromaticAberration((1.001, 0, 0), (0.999, 0, 0))
    on.set(chromatic_aberration=other)
    assert on.chromatic_aberration == other
    with pytest.raises(ValueError):
        on.set(chromatic_aberration=(1, 0, 0))
    on.set(chromatic_aberration=False)
    assert on.chromatic_aberration is None
    for c in calls:
        c.clear()
    b = call(on, kind, t, defects=m)
    assert sum(len(c) for c in calls) == 0
    assert_exact(b.cpu().numpy(), a.cpu().numpy(), f"{cam} {kind} off again")
    off.tonemap_reinhard([a], gamma=0.9)
    on.tonemap_reinhard([b], gamma=0.9)
    assert_exact(on.metrics.cpu().numpy(), off.metrics.cpu().numpy(), "metering")
    off.set(chromatic_aberration=ca)                                          # ... and on
    assert not torch.equal(call(off, kind, t, defects=m), a)


def test_shift_limit_raises_before_any_launch(ti, rng, dev, monkeypatch):
    H, W = 66, 70
    far = math.hypot((H - 1) / 2, (W - 1) / 2)
    over = ti.ChromaticAberration((1 + 8.01 / far, 0, 0))
    calls = [_count_calls(monkeypatch, e) for e in ENTRIES + ["mi_isp_awb_stats_packed", "mi_isp_awb_stats_cfa"]]
    src, x, black, white = source(rng, "p12", H, W)
    t = torch.from_numpy(src).to(dev)
    u = torch.from_numpy(source(rng, "16u", H, W)[0]).to(dev)
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, chromatic_aberration=over, auto_white_balance=True)
    for load in (lambda: isp.load_packed12(t), lambda: isp.load_packed12_batch([t, t]), lambda: isp.load_16u(u),
                 lambda: isp.process_packed12([t]),
                 lambda: ti.chromatic.correct_cfa(torch.zeros((H, W), device=dev), ti.BayerPattern.RGGB, over)):
        with pytest.raises(ValueError, match="chromatic"):
            load()
    assert sum(len(c) for c in calls) == 0
    isp.load_packed12(torch.from_numpy(source(rng, "p12", 6, 4)[0]).to(dev))  # (the same settings fit a small frame)
    # just under the limit: the halo still covers every tap.  With the centre 64 px above (left of) the frame and a scale
    # below 1, rows (columns) 64 and 65 take their taps from 7.7 px inside the tile above (to the left).
    got = capture(monkeypatch, ti.Camera32(ti.BayerPattern.RGGB, device=dev))
    for kw in (dict(), dict(center=(-64.0, 34.5)), dict(center=(32.5, -60.0))):
        cy, cx = kw.get("center", ((H - 1) / 2, (W - 1) / 2))
        far = math.hypot(max(abs(cy), abs(H - 1 - cy)), max(abs(cx), abs(W - 1 - cx)))
        ok = ti.ChromaticAberration((1 - 7.99 / far, 0, 0), (1 + 7.99 / far, 0, 0), **kw)
        assert 7.98 < min(ok.max_shift((H, W))) and max(ok.max_shift((H, W))) < 8
        isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev, chromatic_aberration=ok)
        got.clear()
        isp.load_packed12(t)
        assert_exact(got[0].cpu().numpy(), expected_cfa(isp, x, O.RGGB, "f32")[0], f"a shift of 7.99 px, {kw}")


def test_process_packed12_takes_the_two_calls(ti, rng, dev):
    H, W = 64, 64
    frames = [torch.from_numpy(source(rng, "p12", H, W)[0]).to(dev) for _ in range(3)]
    ca = settings(ti, H, W)
    a = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True, chromatic_aberration=ca)
    b = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True, chromatic_aberration=ca)
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
    """A load + tonemap step with the stage is graph-capturable and replays bit-identically."""
    H, W = 66, 70
    frames = [[torch.from_numpy(source(rng, "p12", H, W)[0]).to(dev) for _ in range(2)] for _ in range(3)]
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64)], (H, W))
    static = [torch.empty_like(f) for f in frames[0]]
    kw = dict(moving_alpha=0.5, device=dev, correct_colors=True, chromatic_aberration=settings(ti, H, W))
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


# ---- batches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("bits", [12, 16])
def test_a_batch_beyond_one_launch(ti, rng, dev, monkeypatch, cam, work, bits):
    """33 frames at 66 x 70 (one launch takes 32): every frame equals its single load, three of them the reference."""
    H, W = 66, 70
    kind = "p12" if bits == 12 else "p16"
    srcs = [source(rng, kind, H, W, levels=True) for _ in range(33)]
    black, white = srcs[0][2:]
    m = seam_defects(ti, rng, H, W)
    isp = getattr(ti, cam)(ti.BayerPattern.BGGR, device=dev, correct_colors=True, black_level=black, white_level=white,
                           chromatic_aberration=settings(ti, H, W), resize_width=36)
    ts = [torch.from_numpy(s[0]).to(dev) for s in srcs]
    fn = isp.load_packed12_batch if bits == 12 else isp.load_packed16_batch
    one = isp.load_packed12 if bits == 12 else isp.load_packed16
    maps = [m if k in (0, 32) else None for k in range(33)]
    got = capture(monkeypatch, isp)
    imgs = fn(ts, defects=maps)
    assert len(got) == 33
    for k in (0, 31, 32):
        want, y = expected_cfa(isp, srcs[k][1], O.BGGR, work, m.mask() if maps[k] is not None else None)
        assert_exact(got[k].cpu().numpy(), want, f"{cam} {kind} batch frame {k} CFA")
        check_image(isp, imgs[k].cpu().numpy(), want, O.BGGR, f"{cam} {kind} batch frame {k}")
    for k in range(33):
        assert torch.equal(imgs[k], one(ts[k], defects=maps[k])), f"frame {k}"


def test_six_full_size_frames_in_one_batch(ti, rng, dev, monkeypatch):
    """Six 4096 x 3072 packed-12 frames in one batch equal their single loads, and the reference on one of them."""
    H, W = 3072, 4096
    codes = rng.integers(0, 4096, (H, W)).astype(np.uint16)
    base = O.encode12(codes)
    frames = [torch.from_numpy(np.ascontiguousarray(np.roll(base, 2 * k, axis=0))).to(dev) for k in range(6)]
    Rn = math.hypot(H / 2, W / 2)
    ca = ti.ChromaticAberration((1 + 2 / Rn, 1.5 / Rn, 2.5 / Rn), (1 - 1 / Rn, -3 / Rn, -1 / Rn))
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, chromatic_aberration=ca, resize_width=512)
    got = capture(monkeypatch, isp)
    imgs = isp.load_packed12_batch(frames)
    cfas = [g for g in got]
    for k in range(6):
        assert torch.equal(imgs[k], isp.load_packed12(frames[k])), f"frame {k}"
        assert torch.equal(got[6 + k], cfas[k]), f"frame {k} CFA"
    x = np.roll(codes, 6, axis=0).astype(f32) * f32(1 / 4095)
    assert_exact(cfas[3].cpu().numpy(), R.route_cfa(x, O.RGGB, ca, "f16"), "frame 3 against the reference")
