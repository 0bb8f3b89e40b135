"""Green equalisation (Camera16/32 green_equalize=, equalize_cfa, the three C entry points) on the GPU against
tests/green_equalize_ref.py.  Every comparison in this file has zero differing bits, NaNs as NaNs.

The route's CFA is captured by wrapping ISP._process_image; it must equal the NumPy f32 contract bit for bit (with the
defect fix-up of tests/test_defects_cpu.py at listed sites), and the loader's image must be O.bayer_to_rgb /
O.resize_bilinear of that CFA bit for bit.  The shapes are written with the kernel's tile (tests/test_green_equalize_cpu.py
holds them to the header): frames smaller than the window, one whole tile, one pixel more on both axes, and an odd width
with a partial last tile on both axes."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chromatic_ref as CR
from tests import denoise_ref as D
from tests import dynamic_defects_ref as DR
from tests import exposure_merge_ref as M
from tests import green_equalize_ref as R
from tests import highlights_ref as HR
from tests import temporal_ref as T
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_denoise import call, capture, loader_x
from tests.test_gpu_shading import PER_SITE, make_grid, pixel_gains
from tests.util import _count_calls, assert_exact

pytestmark = pytest.mark.gpu

TILE_H, TILE_W, MAX_FRAMES = 64, 64, 32
SHAPES = [(2, 2), (3, 5), (6, 6), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (TILE_H + 7, 2 * TILE_W + 3)]
ODD, EVEN = (TILE_H + 7, 2 * TILE_W + 3), (TILE_H + 6, 2 * TILE_W + 4)        # (packed frames are even)
CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]
CCM = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
WB = np.array([1.8, 1.0, 2.1])
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]
FULL = {"p12": 4095, "ids": 4095, "p16": 65535, "16u": 65535, "16f": 1000, "32f": 4095}
GAIN, READ_NOISE = 2.4e-4, 1.5e-3
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def settings(ti, kind="p12", **kw):
    """The settings in the units of the kind's x (load_16f's x is the code, 0 .. 1000; with levels the white level is
    below the codes' top, so x is a little larger: the slope carries it)."""
    return ti.GreenEqualize(threshold=1000 / 256 if kind == "16f" else 1 / 256, **kw)


def encode(kind, codes, levels=False):
    """(the loader's input, x as the loader computes it, black, white) of raw codes in 0 .. FULL[kind]."""
    H, W = codes.shape
    lv = levels and kind in ("p12", "ids", "p16", "16u") and H % 2 == 0 and W % 2 == 0
    black, white = (PER_SITE, FULL[kind] - 195) if lv else (None, None)
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


def source(rng, kind, H, W, pattern, levels=False):
    """(the loader's input, x, black, white) of a generated frame; with levels the codes are laid over the per-site black
    levels, so that x is the scene and not the scene with the blacks' own imbalance."""
    v = R.make_scene(rng, H, W, pattern)
    if levels and kind in ("p12", "ids", "p16", "16u") and H % 2 == 0 and W % 2 == 0:
        b = np.tile(np.reshape(PER_SITE, (2, 2)), (H // 2, W // 2))
        codes = np.rint(b + v * (FULL[kind] - 195 - b)).astype(np.uint16)
    else:
        codes = np.rint(v * FULL[kind]).astype(np.uint16)
    return encode(kind, codes, levels)


def exercised(x, kind, pattern, s, what, mask=None):
    R.assert_exercised(x, pattern, what, excluded=mask, threshold=s.threshold, slope=s.slope, strength=s.strength,
                       radius=s.radius, edge=s.edge)


def expected_cfa(isp, y, work, mask=None):
    """The route's CFA (with the fix-up) of the last stage's y."""
    H, W = y.shape
    grid = isp._applied_shading()
    gain = None if grid is None else pixel_gains(grid.cpu().numpy(), H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        cfa = O.cast_out(y if gain is None else (y * gain).astype(f32), work)
    return cfa if mask is None else correct_cfa(cfa, mask, work)


def check_image(isp, img, cfa, pattern, what):
    H, W = cfa.shape
    rgb = O.bayer_to_rgb(cfa, pattern, correct_colors=isp.color_correct_matrix)
    sz = O.isp_output_size(H, W, isp.resize_width, None)
    assert_exact(img, rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1]), what + " image")


def some_sites(H, W, n=12):
    """n listed sites spread over the frame, green and not, seams included."""
    sites = [(0, 0), (1, 2), (H - 1, W - 1), (H // 2, W // 2), (H // 2 + 1, W // 2), (min(63, H - 1), min(64, W - 1)),
             (min(64, H - 1), min(63, W - 1)), (5, 6), (5, 8), (6, 7), (7, 7), (10, min(40, W - 1))]
    return sorted(set(sites))[:n]


# ---- equalize_cfa ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_equalize_cfa(ti, rng, dev, work, radius, pattern):
    s = ti.GreenEqualize(radius=radius)
    for H, W in SHAPES:
        x = O.cast_out(R.make_frame(rng, H, W, pattern).astype(f32) * f32(1 / 4095), work)
        exercised(x.astype(f32), "p12", pattern, s, f"{H}x{W}")
        want = O.cast_out(R.correct(x.astype(f32), pattern, s), work)
        what = f"{work} R={radius} p{pattern} {H}x{W}"
        got = ti.equalize_cfa(torch.from_numpy(x).to(dev), ti.BayerPattern(pattern), s)
        assert got.device == dev and got.shape == (H, W) and got.dtype == torch.from_numpy(x).dtype
        assert_exact(got.cpu().numpy(), want, what)
        assert not np.array_equal(want, x) or H * W < 4096
    host = ti.equalize_cfa(x, ti.BayerPattern(pattern), s)                    # numpy in, numpy out
    assert isinstance(host, np.ndarray)
    assert_exact(host, want, what + " numpy round trip")
    assert ti.equalize_cfa(np.zeros((0, 8), f32), ti.BayerPattern(pattern)).shape == (0, 8)


@pytest.mark.parametrize("radius", [1, 2])
def test_the_gate_at_equality_and_one_ulp_beyond(ti, dev, radius):
    """|d| == lim applies; with lim the next f32 below (|d| the next f32 above lim) nothing moves."""
    sign = R.phase_sign(O.RGGB, 12, 12)
    x = np.where(sign > 0, 0.5, np.where(sign < 0, 0.25, 0.125)).astype(f32)
    for t in (f32(0.25), np.nextafter(f32(0.25), f32(0))):
        s = ti.GreenEqualize(threshold=float(t), slope=0.0, radius=radius)
        q = R.equalize(x, O.RGGB, threshold=t, slope=0.0, radius=radius)
        assert q.apply[4:8, 4:8][q.green[4:8, 4:8]].all() == (t == f32(0.25)) and q.apply.any() == (t == f32(0.25))
        assert_exact(ti.equalize_cfa(x, ti.BayerPattern.RGGB, s), q.y, f"R={radius} t={t!r}")
    x[sign < 0] = 0.5                                                         # ... and the range gates at range == e
    x[5, 8] = 0.75
    for e in (f32(1), np.nextafter(f32(1), f32(0))):
        s = ti.GreenEqualize(threshold=0.25, slope=0.0, edge=float(e), radius=radius)
        q = R.equalize(x, O.RGGB, threshold=0.25, slope=0.0, edge=e, radius=radius)
        assert q.apply[5, 6] == (e == 1) and q.apply[4, 7] == (e == 1)
        assert_exact(ti.equalize_cfa(x, ti.BayerPattern.RGGB, s), q.y, f"R={radius} edge={e!r}")


@pytest.mark.parametrize("radius", [1, 2])
def test_non_finite_values_as_taps_and_as_centres(ti, rng, dev, radius):
    H, W = ODD
    x = R.make_frame(rng, H, W, O.GBRG).astype(f32) * f32(1 / 4095)
    for k, (r, c) in enumerate(some_sites(H, W) + [(20, 21), (20, 23), (21, 22), (22, 22), (30, 2), (31, 3)]):
        x[r, c] = (np.nan, np.inf, -np.inf)[k % 3]
    s = ti.GreenEqualize(radius=radius)
    q = R.equalize(x, O.GBRG, radius=radius)
    lost = ~np.isfinite(x)
    assert not q.apply[lost].any() and (q.apply & (q.n_o < len(R.taps(radius)[0])) & (q.n_o > 0)).any()
    got = ti.equalize_cfa(x, ti.BayerPattern.GBRG, s)
    assert_exact(got, q.y, f"R={radius} non-finite")
    assert np.array_equal(got[lost].view(np.uint32), x[lost].view(np.uint32))


# ---- the C entry points: every (SRC, OUT) instance ---------------------------------------------------------------------
def raw_kind(kind):
    from taichi_image_amd import _native as N
    return {"p12": N.MI_RAW_PACKED12, "ids": N.MI_RAW_PACKED12, "p16": N.MI_RAW_PACKED16, "16u": N.MI_RAW_16U,
            "16f": N.MI_RAW_16F, "32f": N.MI_RAW_32F}[kind]


@pytest.mark.parametrize("out", ["f16", "f32", "plain"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("radius", [1, 2])
def test_every_instance_of_the_raw_entry(ti, rng, dev, kind, out, radius):
    """mi_isp_green_equalize_raw at one odd shape (packed frames: the even one), without and with levels, a per-site
    grid for the cast outputs and a defect map."""
    from taichi_image_amd import _native as N
    H, W = EVEN if kind in ("p12", "ids", "p16") else ODD
    pattern = PATTERNS[(KINDS.index(kind) + radius) % 4]
    s = settings(ti, kind, radius=radius)
    for extras in (False, True):
        src, x, black, white = source(rng, kind, H, W, pattern, levels=extras)
        grid = make_grid(rng, 5, 7, 4) if extras and out != "plain" else None
        isp = ti.Camera32(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white, lens_shading=grid)
        lv = isp._levels(12 if kind in ("p12", "ids") else 16) if black is not None else None
        m = ti.DefectMap([p for p in some_sites(H, W)], (H, W)) if extras and H % 2 == 0 else None
        mask = None if m is None else m.mask()
        arg = None if m is None else m._arg(dev)
        t = torch.from_numpy(src).to(dev)
        dtype = torch.float16 if out == "f16" else torch.float32
        got = torch.empty((H, W), dtype=dtype, device=dev)
        N.check(N.lib().mi_isp_green_equalize_raw(
            t.data_ptr(), got.data_ptr(), H, W, raw_kind(kind), int(kind == "ids"), N.MI_F16 if out == "f16" else N.MI_F32,
            pattern, lv, N.shading_arg(isp._applied_shading()), arg, s._arg(), int(out == "plain"), N.stream_ptr(dev)))
        what = f"{kind} {out} R={radius} extras={extras}"
        exercised(x, kind, pattern, s, what, mask)
        y = R.correct(x, pattern, s, mask)
        assert not np.array_equal(y, x)
        gain = None if grid is None else pixel_gains(grid, H, W)
        want = y if out == "plain" else O.cast_out(y if gain is None else (y * gain).astype(f32), out)
        assert_exact(got.cpu().numpy(), want, what)


@pytest.mark.parametrize("work", ["f16", "f32"])
def test_a_batch_beyond_one_launch_with_some_maps(ti, rng, dev, work):
    """MAX_FRAMES + 1 tiny frames through the batch entry point, a map for every other one: every frame's CFA, the second
    launch's included."""
    from taichi_image_amd import _native as N
    H, W, n = 6, 10, MAX_FRAMES + 1
    s = ti.GreenEqualize(radius=2)
    m = ti.DefectMap([(1, 2), (2, 3), (4, 6)], (H, W))
    xs = [R.flat_field(rng, H, W, O.BGGR, g=0.1 + 0.02 * k, sigma=0.001) for k in range(n)]
    srcs = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((H, W), dtype=torch.float16 if work == "f16" else torch.float32, device=dev) for _ in range(n)]
    arg = m._arg(dev)
    maps = (ctypes.c_void_p * n)(*[ctypes.addressof(arg) if k % 2 else None for k in range(n)])
    N.check(N.lib().mi_isp_green_equalize_raw_batch(
        N.ptr_array(srcs), N.ptr_array(outs), n, H, W, N.MI_RAW_32F, 0, N.MI_F16 if work == "f16" else N.MI_F32, O.BGGR,
        None, None, maps, s._arg(), 0, N.stream_ptr(dev)))
    for k in range(n):
        q = R.equalize(xs[k], O.BGGR, radius=2, excluded=m.mask() if k % 2 else None)
        assert q.apply.any() and (not k % 2 or not q.apply[1, 2])
        assert_exact(outs[k].cpu().numpy(), O.cast_out(q.y, work), f"{work} frame {k}")


# ---- the loaders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_loader_kind(ti, rng, dev, monkeypatch, cam, work, kind):
    """Every loader through the ISP with the stage alone, with levels, a per-site grid and a DefectMap: a listed tap is
    excluded, a listed centre keeps its value and is replaced by the fix-up afterwards."""
    H, W = EVEN
    pattern = PATTERNS[KINDS.index(kind) % 4]
    s = settings(ti, kind, radius=1 + KINDS.index(kind) % 2)
    src, x, black, white = source(rng, kind, H, W, pattern, levels=True)
    m = ti.DefectMap(some_sites(H, W), (H, W))
    mask = m.mask()
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, color_correction=CCM,
                           black_level=black, white_level=white, lens_shading=make_grid(rng, 5, 7, 4), green_equalize=s)
    n_ge = _count_calls(monkeypatch, "mi_isp_green_equalize_raw_batch")
    got = capture(monkeypatch, isp)
    img = call(isp, kind, torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
    assert len(n_ge) == 1
    what = f"{cam} {kind} p{pattern}"
    exercised(x, kind, pattern, s, what, mask)
    q = R.equalize(x, pattern, excluded=mask, threshold=s.threshold, radius=s.radius)
    assert not q.apply[mask].any() and not np.array_equal(q.y, R.correct(x, pattern, s)), "the map changes nothing"
    want = expected_cfa(isp, q.y, work, mask)
    assert_exact(got[0].cpu().numpy(), want, what + " CFA")
    check_image(isp, img, want, pattern, what)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("bits", [12, 16])
def test_batch_loaders_with_per_frame_maps(ti, rng, dev, monkeypatch, cam, work, bits):
    H, W = EVEN
    kind = "p12" if bits == 12 else "p16"
    s = settings(ti, kind, radius=2)
    srcs = [source(rng, kind, H, W, O.BGGR, levels=True) for _ in range(3)]
    black, white = srcs[0][2:]
    m = ti.DefectMap(some_sites(H, W), (H, W))
    isp = getattr(ti, cam)(ti.BayerPattern.BGGR, device=dev, correct_colors=True, black_level=black, white_level=white,
                           green_equalize=s, resize_width=36)
    got = capture(monkeypatch, isp)
    fn = isp.load_packed12_batch if bits == 12 else isp.load_packed16_batch
    imgs = fn([torch.from_numpy(f[0]).to(dev) for f in srcs], defects=[m, None, m])
    for k, (f, im) in enumerate(zip(srcs, imgs)):
        mask = m.mask() if k != 1 else None
        want = expected_cfa(isp, R.correct(f[1], O.BGGR, s, mask), work, mask)
        assert_exact(got[k].cpu().numpy(), want, f"{cam} {kind} batch frame {k} CFA")
        check_image(isp, im.cpu().numpy(), want, O.BGGR, f"{cam} {kind} batch frame {k}")


@pytest.mark.parametrize("cam,work", CAMS)
def test_a_bracket_loader_behind_exposure_merge(ti, rng, dev, monkeypatch, cam, work):
    """Exposure merge -> green equalisation through a bracket loader: the stage sees the merged frame."""
    from tests.test_gpu_exposure_merge import load, to_dev
    H, W, ratios, kind, pattern = EVEN[0], EVEN[1], (1, 4), "p12", O.RGGB
    em = ti.ExposureMerge(ratios, GAIN, READ_NOISE, saturation=0.9)
    s = settings(ti, kind)
    sign = R.phase_sign(pattern, H, W)
    srcs, xs = [], []
    for u in M.make_bracket(rng, H, W, ratios, GAIN, READ_NOISE):
        src, x, _, _ = encode(kind, np.rint(np.clip(u * (1.0 + 0.02 * sign), 0, 1) * FULL[kind]).astype(np.uint16))
        srcs.append(src)
        xs.append(x)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, lens_shading=make_grid(rng, 3, 4, 1),
                           exposure_merge=em, green_equalize=s)
    counts = [_count_calls(monkeypatch, e) for e in ("mi_isp_merge_raw_batch", "mi_isp_green_equalize_raw_batch")]
    got = capture(monkeypatch, isp)
    img = load(isp, kind, to_dev(srcs, dev)).cpu().numpy()
    assert [len(c) for c in counts] == [1, 1]
    merged = M.merge(xs, em, None)
    q = R.equalize(merged, pattern, threshold=s.threshold)
    assert q.apply[q.green].mean() > 0.1
    want = expected_cfa(isp, q.y, work)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} merge in front CFA")
    check_image(isp, img, want, pattern, f"{cam} merge in front")


# ---- the stage behind the others ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u", "32f"])
def test_behind_raw_denoise(ti, rng, dev, monkeypatch, cam, work, kind):
    """Raw noise reduction -> green equalisation: the filter writes its f32 y without a grid (within its own bound of its
    reference), and the CFA is the contract on exactly that y."""
    from tests.test_gpu_raw_stage_matrix import record_outputs
    H, W = EVEN
    pattern = O.GRBG
    src, x, black, white = source(rng, kind, H, W, pattern, levels=True)
    dn = ti.RawDenoise(0.002, 0.01, strength=1.5, radius=1)
    m = ti.DefectMap(some_sites(H, W), (H, W))
    mask = m.mask()
    s = settings(ti, kind)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, black_level=black, white_level=white,
                           lens_shading=make_grid(rng, 5, 7, 4), raw_denoise=dn, green_equalize=s)
    wrote = record_outputs(monkeypatch, "mi_isp_denoise_raw_batch", 1)
    counts = [_count_calls(monkeypatch, e) for e in ("mi_isp_denoise_raw_batch", "mi_isp_green_equalize_raw_batch")]
    got = capture(monkeypatch, isp)
    img = call(isp, kind, torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
    assert [len(c) for c in counts] == [1, 1] and len(wrote) == 1
    y_dn = wrote[0][0].cpu().numpy()
    assert y_dn.dtype == f32
    D.assert_within_bound(y_dn, D.route_yg(x, dn, None, mask), "f32", f"{cam} {kind} the filter's y", where=~mask)
    q = R.equalize(y_dn, pattern, excluded=mask, threshold=s.threshold)
    assert q.apply[q.green].mean() > 0.25
    want = expected_cfa(isp, q.y, work, mask)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} {kind} behind denoise CFA")
    check_image(isp, img, want, pattern, f"{cam} {kind} behind denoise")


@pytest.mark.parametrize("kind", ["p12", "32f"])
def test_behind_temporal_denoise(ti, rng, dev, monkeypatch, kind):
    """Temporal noise reduction -> green equalisation over three frames: the history holds the values BEFORE the
    equalisation, the CFA the equalised blend."""
    H, W = EVEN
    pattern = O.RGGB
    tn = ti.TemporalDenoise(GAIN, READ_NOISE)
    s = settings(ti, kind)
    isp = ti.Camera16(ti.BayerPattern(pattern), device=dev, temporal_denoise=tn, green_equalize=s,
                      lens_shading=make_grid(rng, 3, 4, 1))
    got = capture(monkeypatch, isp)
    hist = ti.TemporalHistory()
    h = None
    base = R.make_scene(rng, H, W, pattern)
    for k in range(3):
        noisy = np.clip(base + rng.normal(0, 0.002, (H, W)), 0, 1)
        src, x, _, _ = encode(kind, np.rint(noisy * FULL[kind]).astype(np.uint16))
        h = T.blend(x, h, tn)
        y = R.correct(h, pattern, s)
        got.clear()
        call(isp, kind, torch.from_numpy(src).to(dev), history=hist)
        assert_exact(hist.plane.cpu().numpy(), h, f"{kind} frame {k} history")
        assert_exact(got[0].cpu().numpy(), expected_cfa(isp, y, "f16"), f"{kind} frame {k} CFA")
        assert not np.array_equal(y, h)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "32f"])
def test_behind_dynamic_defects_highlights_and_chromatic_aberration(ti, rng, dev, monkeypatch, cam, work, kind):
    """Dynamic defects -> highlight reconstruction -> chromatic aberration -> green equalisation, with a DefectMap and
    automatic white balance off / on the colour matrix: composed from the stages' references in _raw_chain's order."""
    H, W = EVEN
    pattern = O.GBRG
    codes = R.make_frame(rng, H, W, pattern, FULL[kind])
    codes[8:12, 20:26] = FULL[kind]                                           # a clipped blob
    codes[30, 11] = FULL[kind]                                                # a hot pixel
    src, x, black, white = encode(kind, codes)
    m = ti.DefectMap(some_sites(H, W), (H, W))
    mask = m.mask()
    k = CR.frame_settings(H, W)
    dd, hl, ca = ti.DynamicDefects(), ti.Highlights("rebuild", 0.98), ti.ChromaticAberration(k.red, k.blue)
    s = settings(ti, kind, radius=2)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, white_balance=WB,
                           lens_shading=make_grid(rng, 5, 7, 4), dynamic_defects=dd, highlights=hl,
                           chromatic_aberration=ca, green_equalize=s)
    names = ("mi_isp_dynamic_defects_raw_batch", "mi_isp_highlights_raw_batch", "mi_isp_chromatic_raw_batch",
             "mi_isp_green_equalize_raw_batch")
    counts = [_count_calls(monkeypatch, e) for e in names]
    got = capture(monkeypatch, isp)
    img = call(isp, kind, torch.from_numpy(src).to(dev), defects=m).cpu().numpy()
    assert [len(c) for c in counts] == [1, 1, 1, 1]
    y1 = DR.correct(x, dd, mask)
    y2 = HR.reconstruct(y1, pattern, f32(WB), "rebuild", 0.98, mask)
    y3 = CR.correct(y2, pattern, ca, mask)
    q = R.equalize(y3, pattern, excluded=mask, threshold=s.threshold, radius=2)
    assert not np.array_equal(y1, x) and not np.array_equal(y2, y1) and not np.array_equal(y3, y2) and q.apply.mean() > 0.1
    want = expected_cfa(isp, q.y, work, mask)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} {kind} chain CFA")
    check_image(isp, img, want, pattern, f"{cam} {kind} chain")


@pytest.mark.parametrize("cam,work", CAMS)
def test_with_auto_white_balance(ti, rng, dev, cam, work):
    """With AWB on the grid the stage applies is the AWB gains': the image equals what an ISP without the stage makes of
    the reference's y given as an f32 frame (the same statistics: AWB meters x before any raw stage... of its own load)."""
    H, W = EVEN
    pattern = O.RGGB
    src, x, _, _ = source(rng, "32f", H, W, pattern)
    s = ti.GreenEqualize()
    kw = dict(device=dev, correct_colors=True, auto_white_balance=ti.AutoWhiteBalance())
    on = getattr(ti, cam)(ti.BayerPattern(pattern), green_equalize=s, **kw)
    off = getattr(ti, cam)(ti.BayerPattern(pattern), **kw)
    t = torch.from_numpy(src).to(dev)
    a = on.load_32f(t)
    gains = on._applied_shading().cpu().numpy()
    y = R.correct(x, pattern, s)
    want = O.cast_out((y * pixel_gains(gains, H, W)).astype(f32), work)
    rgb = O.bayer_to_rgb(want, pattern, correct_colors=on.color_correct_matrix)
    assert_exact(a.cpu().numpy(), rgb, f"{cam} AWB image")
    assert not torch.equal(a, off.load_32f(t))


@pytest.mark.parametrize("cam,work", CAMS)
def test_directional_demosaic_and_antialiased_resize(ti, rng, dev, monkeypatch, cam, work):
    """The stage in front of the other demosaic and the other resize: the image is what an ISP without the stage makes of
    the reference's y."""
    H, W = EVEN
    src, x, _, _ = source(rng, "p12", H, W, O.GRBG)
    s = ti.GreenEqualize()
    y = R.correct(x, O.GRBG, s)
    for kw in (dict(demosaic=ti.Demosaic("directional")), dict(resample=ti.Resample("lanczos3"), resize_width=36),
               dict(demosaic=ti.Demosaic("directional"), resample=ti.Resample("area"), scale=0.5)):
        isp = getattr(ti, cam)(ti.BayerPattern.GRBG, device=dev, correct_colors=True, green_equalize=s, **kw)
        plain = getattr(ti, cam)(ti.BayerPattern.GRBG, device=dev, correct_colors=True, **kw)
        got = capture(monkeypatch, isp)
        img = isp.load_packed12(torch.from_numpy(src).to(dev))
        want = plain.load_32f(torch.from_numpy(y).to(dev))
        if got:                                                                # (the routes that go through _process_image)
            assert_exact(got[0].cpu().numpy(), O.cast_out(y, work), f"{cam} {sorted(kw)} CFA")
        assert_exact(img.cpu().numpy(), want.cpu().numpy(), f"{cam} {sorted(kw)} image")
        assert not torch.equal(img, plain.load_packed12(torch.from_numpy(src).to(dev))), "the stage did not matter"
        monkeypatch.undo()


# ---- on and off --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u", "32f"])
def test_set_turns_it_on_and_off(ti, rng, dev, monkeypatch, cam, work, kind):
    """set(green_equalize=...) turns the stage on; set(green_equalize=False) gives back the bits - images and metering -
    and the launches of an ISP that never had the option."""
    from taichi_image_amd import _native as N
    H, W = EVEN
    src, x, black, white = source(rng, kind, H, W, O.GBRG, levels=True)
    m = ti.DefectMap(some_sites(H, W), (H, W))
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white,
              lens_shading=make_grid(rng, 5, 7, 4), resize_width=36, raw_denoise=ti.RawDenoise(0.002, 0.01))
    off = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw)
    on = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw)
    t = torch.from_numpy(src).to(dev)
    assert on.green_equalize is None
    on.set(green_equalize=settings(ti, kind))
    assert on.green_equalize == settings(ti, kind)
    a = call(off, kind, t, defects=m)
    assert not torch.equal(call(on, kind, t, defects=m), a), "the stage must matter"
    on.set(moving_alpha=0.2)                                                  # (None leaves it)
    assert on.green_equalize is not None
    on.set(green_equalize=False)
    assert on.green_equalize is None
    off.set(moving_alpha=0.2)
    names = [n for n in N.SIGNATURES if n != "mi_isp_last_error"]             # every entry point of the library
    counts = {n: _count_calls(monkeypatch, n) for n in names}
    b = call(on, kind, t, defects=m)
    seen_on = {n: len(c) for n, c in counts.items()}
    a = call(off, kind, t, defects=m)
    seen_off = {n: len(c) - seen_on[n] for n, c in counts.items()}
    assert seen_on == seen_off and seen_on["mi_isp_green_equalize_raw_batch"] == 0 and sum(seen_on.values()) >= 2
    assert_exact(b.cpu().numpy(), a.cpu().numpy(), f"{cam} {kind} off again")
    off.tonemap_reinhard([a], gamma=0.9)
    on.tonemap_reinhard([b], gamma=0.9)
    assert_exact(on.metrics.cpu().numpy(), off.metrics.cpu().numpy(), "metering")
    with pytest.raises(ValueError):
        on.set(green_equalize=True)


def test_process_packed12_takes_the_two_calls(ti, rng, dev):
    H, W = TILE_H, TILE_W
    frames = [torch.from_numpy(source(rng, "p12", H, W, O.RGGB)[0]).to(dev) for _ in range(3)]
    s = ti.GreenEqualize()
    plain = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True)
    a = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True, green_equalize=s)
    b = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True, green_equalize=s)
    assert not torch.equal(plain.load_packed12_batch(frames)[0], b.load_packed12_batch(frames)[0])
    for step in range(2):
        outs, imgs = a.process_packed12(frames, gamma=0.7, keep_images=True)
        ref_imgs = b.load_packed12_batch(frames)
        ref_outs = b.tonemap_reinhard(ref_imgs, gamma=0.7)
        for o, r in zip(outs, ref_outs):
            assert_exact(o.cpu().numpy(), r.cpu().numpy(), f"step {step} u8")
        for i, r in zip(imgs, ref_imgs):
            assert_exact(i.cpu().numpy(), r.cpu().numpy(), f"step {step} images")
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), f"step {step} metering state")


# ---- a visible result --------------------------------------------------------------------------------------------------
def test_the_checkerboard_falls(ti, dev):
    """The flat +-2 % field through the 13-tap demosaic with the stage off and on: the green channel's checkerboard
    amplitude (half the mean difference between the green channel at the two green phases' sites) falls."""
    H, W = 128, 128
    x = R.flat_field(np.random.default_rng(0), H, W, O.RGGB, 0.25, 0.02, 0.0)
    sign = R.phase_sign(O.RGGB, H, W)
    t = torch.from_numpy(x).to(dev)
    amp = {}
    for name, s in (("off", None), ("on", ti.GreenEqualize())):
        isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev, green_equalize=s)
        g = isp.load_32f(t).cpu().numpy()[8:-8, 8:-8, 1].astype(np.float64)
        sg = sign[8:-8, 8:-8]
        amp[name] = abs(g[sg > 0].mean() - g[sg < 0].mean()) / 2
    print(f"green checkerboard amplitude: off {amp['off']:.3e}, on {amp['on']:.3e}")
    assert amp["on"] < amp["off"]
