"""Temporal noise reduction (Camera16/32 temporal_denoise= and history=, temporal_cfa, the three C entries) on the GPU
against tests/temporal_ref.py.

The route's CFA is captured by wrapping ISP._process_image; it and the new history plane must equal the NumPy f32 contract
bit for bit (with the defect fix-up of tests/test_defects_cpu.py at listed sites), and the loader's image must be
O.bayer_to_rgb / O.resize_bilinear of that CFA bit for bit.  The tile is 64 x 64 and the halo 2: the shapes are the
smallest that reach every seam.  The frames (temporal_ref.make_sequence) put every weight class in a frame, which the
reference alone asserts."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chromatic_ref as CR
from tests import denoise_ref as D
from tests import highlights_ref as HR
from tests import temporal_ref as T
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
ENTRIES = ["mi_isp_temporal_raw", "mi_isp_temporal_raw_batch", "mi_isp_temporal_cfa"]
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
    """The noise model of the generated frames in the units of the kind's x (load_16f's x is the code, 0 .. 1000)."""
    scale = 1000.0 if kind == "16f" else 1.0
    return ti.TemporalDenoise(GAIN * scale, READ_NOISE * scale, **kw)


def encode(kind, u, levels=False):
    """(the loader's input, x as the loader computes it, black, white) of the values u in [0, 1]."""
    lv = levels and kind in ("p12", "ids", "p16", "16u")
    full = {"p12": 4095, "ids": 4095, "p16": 65535, "16u": 65535, "16f": 1000, "32f": 1}[kind]
    black, white = (PER_SITE, full - 195) if lv else (None, None)
    if kind == "32f":
        src = codes = u.astype(f32)
    else:
        codes = np.rint(u * full).astype(np.uint16)
        if lv:                                                # (the values are x: the codes carry the levels)
            b = np.tile(np.reshape(black, (2, 2)), (u.shape[0] // 2, u.shape[1] // 2))
            codes = np.rint(u * (white - b) + b).astype(np.uint16)
        src = codes
        if kind in ("p12", "ids"):
            src = O.encode12(codes, ids_format=kind == "ids")
            codes = O.decode12(src, "u16", ids_format=kind == "ids")      # (the IDS packing does not round-trip)
        elif kind == "p16":
            src = codes.view(np.uint8).reshape(u.shape[0], 2 * u.shape[1])
    return src, loader_x(kind, codes, black, white), black, white


def sequence(rng, kind, H, W, n, levels=False):
    """n frames of one camera: ([the loader's inputs], [their x], black, white)."""
    out = [encode(kind, u, levels) for u in T.make_sequence(rng, H, W, n, GAIN, READ_NOISE)]
    return [o[0] for o in out], [o[1] for o in out], out[0][2], out[0][3]


def assert_exercised(x, h, s, mask, what):
    """On the reference alone: a frame of 4096 pixels or more has 10 % of its pixels in each weight class, and every pixel
    with w > 0 and h != x changes."""
    if x.size >= 4096:
        none, some, most, changes = T.coverage(x, h, s, mask)
        assert min(none, some, most) >= 0.10, f"{what}: the frame does not exercise the operator ({none}, {some}, {most})"
        assert changes, f"{what}: a pixel with w > 0 and h != x keeps its value"


def cfa_of(isp, y, work, mask=None):
    """The route's CFA (with the fix-up) of the stage's y."""
    H, W = y.shape
    grid = isp._applied_shading()
    gain = None if grid is None else pixel_gains(grid.cpu().numpy(), H, W)
    cfa = O.cast_out(y if gain is None else (y * gain).astype(f32), work)
    return cfa if mask is None else correct_cfa(cfa, mask, work)


def check_image(isp, img, cfa, pattern, what):
    H, W = cfa.shape
    rgb = O.bayer_to_rgb(cfa, pattern, correct_colors=isp.color_correct_matrix)
    sz = O.isp_output_size(H, W, isp.resize_width, None)
    assert_exact(img, rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1]), what + " image")


def seam_defects(ti, rng, H, W):
    """A defect map with sites at the corners, on both sides of the tile seams and scattered: listed centres and listed
    taps of their neighbours, clusters of same-site neighbours included."""
    sites = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (1, 1), (H - 2, W - 2)}
    for r, c in [(58, 60), (62, 62), (64, 64), (63, 65), (66, 60), (20, 62), (62, 20)]:
        if r + 2 < H and c + 2 < W:
            sites |= {(r, c), (r, c + 2), (r + 2, c), (r + 2, c + 2)}
    sites |= {(int(r), int(c)) for r, c in zip(rng.integers(0, H, 60), rng.integers(0, W, 60))}
    return ti.DefectMap(sorted(sites), (H, W))


# ---- temporal_cfa ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
def test_temporal_cfa(ti, rng, dev, work):
    s = settings(ti)
    for H, W in SHAPES + [(1, 5), (3, 1), (65, 67)]:
        xs = [O.cast_out(u.astype(f32), work) for u in T.make_sequence(rng, H, W, 3, GAIN, READ_NOISE)]
        hist, host_hist = ti.TemporalHistory(), ti.TemporalHistory()
        h = None
        for k, x in enumerate(xs):
            want_y = T.blend(x.astype(f32), h, s)
            if k == 1:
                assert_exercised(x.astype(f32), h, s, None, f"{work} {H}x{W}")
            got = ti.temporal_cfa(torch.from_numpy(x).to(dev), hist, s)
            assert got.device == dev and got.shape == (H, W) and hist.frames == k + 1 and hist.shape == (H, W)
            assert_exact(got.cpu().numpy(), O.cast_out(want_y, work), f"{work} {H}x{W} frame {k}")
            assert_exact(hist.plane.cpu().numpy(), want_y, f"{work} {H}x{W} frame {k} history")
            host = ti.temporal_cfa(x, host_hist, s)                        # numpy in, numpy out
            assert isinstance(host, np.ndarray)
            assert_exact(host, O.cast_out(want_y, work), "numpy round trip")
            h = want_y
    empty = ti.temporal_cfa(np.zeros((0, 8), f32), ti.TemporalHistory(), s)
    assert empty.shape == (0, 8)


@pytest.mark.parametrize("H,W", [(66, 70), (130, 66)])
def test_every_rounding_and_the_order_of_the_sum(ti, rng, dev, H, W):
    """A frame whose weights are almost all partial and whose differences span the whole range: y follows every rounding
    of the metric, the order of its sum included (tests/test_temporal_cpu.py shows that the reversed order changes more
    than 5 % of this frame).  Through temporal_cfa, and through load_32f with a defect map."""
    x, h, args = T.rounding_frame(rng, H, W)
    s = ti.TemporalDenoise(*args)
    assert (T.blend(x, h, s) != T.blend(x, h, s, taps=T.TAPS[::-1])).mean() > 0.05
    for mask_map in (None, seam_defects(ti, rng, H, W)):
        mask = None if mask_map is None else mask_map.mask()
        isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev, temporal_denoise=s)
        zero = ti.Camera32(ti.BayerPattern.RGGB, device=dev, temporal_denoise=ti.TemporalDenoise(args[0], args[1], args[2], 0.0))
        hist = ti.TemporalHistory()
        zero.load_32f(torch.from_numpy(h).to(dev), history=hist)              # (max_weight 0: the history is h itself)
        assert_exact(hist.plane.cpu().numpy(), h, "the seeded history")
        isp.load_32f(torch.from_numpy(x).to(dev), defects=mask_map, history=hist)
        assert_exact(hist.plane.cpu().numpy(), T.blend(x, h, s, mask), f"{H}x{W} map={mask_map is not None}")
    hist = ti.TemporalHistory()
    ti.temporal_cfa(torch.from_numpy(h).to(dev), hist, s)
    got = ti.temporal_cfa(torch.from_numpy(x).to(dev), hist, s)
    assert_exact(got.cpu().numpy(), T.blend(x, h, s), f"{H}x{W} temporal_cfa")


# ---- the loaders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_source_kind_and_shape(ti, rng, dev, monkeypatch, cam, work, kind):
    """Every source kind and both work dtypes at every shape, three consecutive frames through one history; levels and a
    per-site grid at the seam shapes."""
    s = settings(ti, kind)
    for i, (H, W) in enumerate(SHAPES):
        pattern = i % 4
        extras = H * W >= 4096 and (i & 1) == 0
        srcs, xs, black, white = sequence(rng, kind, H, W, 3, levels=extras)
        grid = make_grid(rng, 5, 7, 4) if extras else None
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, color_correction=CCM,
                               black_level=black, white_level=white, lens_shading=grid, temporal_denoise=s)
        got = capture(monkeypatch, isp)
        hist = ti.TemporalHistory()
        h = None
        for k, (src, x) in enumerate(zip(srcs, xs)):
            what = f"{cam} {kind} p{pattern} {H}x{W} extras={extras} frame {k}"
            y = T.blend(x, h, s)
            if k == 1:
                assert_exercised(x, h, s, None, what)
            got.clear()
            img = call(isp, kind, torch.from_numpy(src).to(dev), history=hist).cpu().numpy()
            want = cfa_of(isp, y, work)
            assert_exact(got[0].cpu().numpy(), want, what + " CFA")
            assert_exact(hist.plane.cpu().numpy(), y, what + " history")
            assert hist.frames == k + 1
            check_image(isp, img, want, pattern, what)
            h = y
        if H * W >= 4096:                                     # the third output depends on the first frame
            assert not np.array_equal(h, T.run(xs[1:], s)[-1])


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_awb_gains_a_grid_and_a_defect_map(ti, rng, dev, monkeypatch, cam, work, kind):
    """AWB on (the effective grid E is the gain, the statistics read the source), levels, and a defect map with listed
    centres and listed taps: a listed site never feeds a neighbour's metric and is itself replaced by the fix-up."""
    H, W = 66, 70
    pattern = O.GBRG
    s = settings(ti, kind)
    srcs, xs, black, white = sequence(rng, kind, H, W, 2, levels=True)
    m = seam_defects(ti, rng, H, W)
    mask = m.mask()
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white, auto_white_balance=True,
              moving_alpha=0.5, lens_shading=make_grid(rng, 5, 7, 4))
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), temporal_denoise=s, **kw)
    plain = getattr(ti, cam)(ti.BayerPattern(pattern), **kw)
    hist = ti.TemporalHistory()
    ts = [torch.from_numpy(src).to(dev) for src in srcs]
    call(isp, kind, ts[0], defects=m, history=hist)
    call(plain, kind, ts[0], defects=m)
    assert_exact(isp._awb_pending.cpu().numpy(), plain._awb_pending.cpu().numpy(), "pending statistics")
    isp.update_white_balance()
    assert not np.array_equal(isp._awb_gains.cpu().numpy(), f32(WB)), "the update left the seed"
    assert_exact(hist.plane.cpu().numpy(), xs[0], "the history holds values before any gain")
    got = capture(monkeypatch, isp)
    img = call(isp, kind, ts[1], defects=m, history=hist).cpu().numpy()
    y = T.blend(xs[1], xs[0], s, mask)
    assert_exercised(xs[1], xs[0], s, mask, f"{cam} {kind}")
    assert not np.array_equal(y, T.blend(xs[1], xs[0], s)), "the map changes no weight: the case shows nothing"
    want = cfa_of(isp, y, work, mask)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} {kind} awb + defects CFA")
    assert_exact(hist.plane.cpu().numpy(), y, f"{cam} {kind} awb + defects history")
    check_image(isp, img, want, pattern, f"{cam} {kind} awb + defects")


# ---- the C entries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
def test_c_entries_single_batch_and_plain(ti, rng, dev, work):
    """mi_isp_temporal_raw with the plain output and a NULL CFA writes the history once; a batch of three frames in one
    launch, one of them with an empty history, equals three single calls."""
    from taichi_image_amd import _native
    L, stream = _native.lib(), _native.stream_ptr(dev)
    H, W = 66, 70
    s = settings(ti)
    code = _native.MI_F16 if work == "f16" else _native.MI_F32
    tdt = torch.float16 if work == "f16" else torch.float32
    m = seam_defects(ti, rng, H, W)
    mask, arg = m.mask(), m._arg(dev)
    cams = []
    for k in range(3):
        us = T.make_sequence(rng, H, W, 2, GAIN, READ_NOISE)
        h, x = us[0].astype(f32), us[1].astype(f32)
        cams.append((None if k == 1 else h, x))               # the second camera's history is empty
    new = lambda dt=torch.float32: torch.empty((H, W), dtype=dt, device=dev)  # noqa: E731
    xs = [torch.from_numpy(x).to(dev) for _, x in cams]
    hs = [None if h is None else torch.from_numpy(h).to(dev) for h, _ in cams]
    wants = [T.blend(x, h, s, mask) for h, x in cams]
    assert_exercised(cams[0][1], cams[0][0], s, mask, "C entries")
    # single calls: the CFA form and the plain, single-write form
    singles = []
    for k in range(3):
        ho, cfa, hp = new(), new(tdt), new()
        hin = None if hs[k] is None else hs[k].data_ptr()
        _native.check(L.mi_isp_temporal_raw(xs[k].data_ptr(), hin, ho.data_ptr(), cfa.data_ptr(), H, W, _native.MI_RAW_32F, 0,
                                            code, None, None, arg, s._arg(), 0, stream))
        _native.check(L.mi_isp_temporal_raw(xs[k].data_ptr(), hin, hp.data_ptr(), None, H, W, _native.MI_RAW_32F, 0,
                                            code, None, None, arg, s._arg(), 1, stream))
        assert_exact(ho.cpu().numpy(), wants[k], f"single {k} history")
        assert_exact(hp.cpu().numpy(), wants[k], f"single {k} plain y")
        assert_exact(cfa.cpu().numpy(), O.cast_out(wants[k], work), f"single {k} CFA")
        singles.append((ho, cfa))
    # one launch
    hos, cfas = [new() for _ in range(3)], [new(tdt) for _ in range(3)]
    p_hin = (ctypes.c_void_p * 3)(*[None if h is None else h.data_ptr() for h in hs])
    p_maps = (ctypes.c_void_p * 3)(*[ctypes.addressof(arg)] * 3)
    _native.check(L.mi_isp_temporal_raw_batch(_native.ptr_array(xs), p_hin, _native.ptr_array(hos), _native.ptr_array(cfas), 3,
                                              H, W, _native.MI_RAW_32F, 0, code, None, None, p_maps, s._arg(), 0, stream))
    for k in range(3):
        assert_exact(hos[k].cpu().numpy(), singles[k][0].cpu().numpy(), f"batch {k} history")
        assert_exact(cfas[k].cpu().numpy(), singles[k][1].cpu().numpy(), f"batch {k} CFA")
    assert_exact(hos[1].cpu().numpy(), cams[1][1], "an empty history gives y = x")
    # all histories empty: a NULL list
    _native.check(L.mi_isp_temporal_raw_batch(_native.ptr_array(xs), None, _native.ptr_array(hos), None, 3, H, W,
                                              _native.MI_RAW_32F, 0, code, None, None, None, s._arg(), 1, stream))
    for k in range(3):
        assert_exact(hos[k].cpu().numpy(), cams[k][1], f"no history {k}")
    # mi_isp_temporal_cfa
    x = O.cast_out(cams[0][1], work)
    out, ho = new(tdt), new()
    _native.check(L.mi_isp_temporal_cfa(torch.from_numpy(x).to(dev).data_ptr(), hs[0].data_ptr(), ho.data_ptr(),
                                        out.data_ptr(), H, W, code, s._arg(), stream))
    want = T.blend(x.astype(f32), cams[0][0], s)
    assert_exact(ho.cpu().numpy(), want, "temporal_cfa history")
    assert_exact(out.cpu().numpy(), O.cast_out(want, work), "temporal_cfa CFA")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("bits", [12, 16])
def test_batch_loaders_equal_single_loads(ti, rng, dev, monkeypatch, cam, work, bits):
    """Three cameras in one load_packed*_batch call, one of them with an empty history and one with a defect map, give the
    bits of three single loads - images and histories - in ONE launch of the stage."""
    H, W = 66, 70
    kind = "p12" if bits == 12 else "p16"
    s = settings(ti)
    kw = dict(device=dev, correct_colors=True, lens_shading=make_grid(rng, 3, 4, 1), temporal_denoise=s)
    a = getattr(ti, cam)(ti.BayerPattern.GRBG, **kw)
    b = getattr(ti, cam)(ti.BayerPattern.GRBG, **kw)
    m = seam_defects(ti, rng, H, W)
    seqs = [[torch.from_numpy(f).to(dev) for f in sequence(rng, kind, H, W, 2)[0]] for _ in range(3)]
    ha, hb = [ti.TemporalHistory() for _ in range(3)], [ti.TemporalHistory() for _ in range(3)]
    load_a = a.load_packed12_batch if bits == 12 else a.load_packed16_batch
    load_b = b.load_packed12 if bits == 12 else b.load_packed16
    maps = [None, m, None]
    for k in (0, 2):                                          # cameras 0 and 2 have seen a frame, camera 1 has not
        load_a([seqs[k][0]], history=[ha[k]])
        load_b(seqs[k][0], history=hb[k])
    n = _count_calls(monkeypatch, "mi_isp_temporal_raw_batch")
    imgs = load_a([q[1] for q in seqs], defects=maps, history=ha)
    assert len(n) == 1
    for k in range(3):
        ref = load_b(seqs[k][1], defects=maps[k], history=hb[k])
        assert_exact(imgs[k].cpu().numpy(), ref.cpu().numpy(), f"{cam} {bits} camera {k} image")
        assert_exact(ha[k].plane.cpu().numpy(), hb[k].plane.cpu().numpy(), f"{cam} {bits} camera {k} history")
        assert ha[k].frames == hb[k].frames == (1 if k == 1 else 2)
    assert not torch.equal(ha[0].plane, ha[2].plane)


# ---- exact properties, chains, state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_max_weight_zero_is_the_load_without_the_stage(ti, rng, dev, cam, work, kind):
    """max_weight = 0 gives the bits of the same load without the stage: levels, shading, AWB, defects, the resize, a lens."""
    H, W = 66, 70
    srcs, xs, black, white = sequence(rng, kind, H, W, 2, levels=True)
    m = seam_defects(ti, rng, H, W)
    K = np.array([[60.0, 0, W / 2 - 3], [0, 62.0, H / 2 + 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, (-0.2, 0.05, 0.001, -0.002), (H, W))
    for extra in (dict(resize_width=36), dict(scale=0.5, lens=lens)):
        lens_kw = dict(undistort=extra.pop("lens")) if "lens" in extra else {}
        kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white, auto_white_balance=True,
                  lens_shading=make_grid(rng, 5, 7, 4), **extra)
        on = getattr(ti, cam)(ti.BayerPattern.GBRG, temporal_denoise=settings(ti, kind, max_weight=0.0), **kw)
        off = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw)
        hist = ti.TemporalHistory()
        for k, src in enumerate(srcs):
            t = torch.from_numpy(src).to(dev)
            a = call(on, kind, t, defects=m, history=hist, **lens_kw)
            b = call(off, kind, t, defects=m, **lens_kw)
            assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"{cam} {kind} {extra} frame {k}")
            assert_exact(hist.plane.cpu().numpy(), xs[k], f"{cam} {kind} {extra} history {k}")
        assert_exact(on._awb_pending.cpu().numpy(), off._awb_pending.cpu().numpy(), "pending statistics")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_chain_of_all_four_raw_stages(ti, rng, dev, monkeypatch, cam, work, kind):
    """Highlights -> chromatic aberration -> temporal -> raw denoise on the second frame of a history: the references
    applied in that order.  The temporal stage's y (the history) is bit-exact; the final CFA holds the denoise filter's own
    bound (tests/denoise_ref.py) against the NumPy chain."""
    H, W = 66, 70
    pattern = O.GRBG
    full = {"p12": 4095, "16u": 65535}[kind]
    s = settings(ti)
    dn = ti.RawDenoise(0.002, 0.01, strength=1.5, radius=1)
    hl = ti.Highlights("rebuild", 0.98)
    ca = ti.ChromaticAberration((1.01, -0.02, 0.005), (0.992, 0.015, 0.0))
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64), (65, 69), (33, 0), (60, 62), (62, 66), (64, 58)], (H, W))
    mask = m.mask()
    grid = make_grid(rng, 5, 7, 4)
    # two frames: clipped blobs (for highlights) on the generated sequence
    us = T.make_sequence(rng, H, W, 2, GAIN, READ_NOISE)
    blobs = HR.make_codes(rng, H, W, full, int(0.985 * full) + 1, pattern) >= int(0.985 * full) + 1
    srcs, xs = [], []
    for u in us:
        codes = np.where(blobs, full, np.rint(u * full)).astype(np.uint16)
        srcs.append(O.encode12(codes) if kind == "p12" else codes)
        xs.append(loader_x(kind, codes, None, None))
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, lens_shading=grid, raw_denoise=dn,
                           highlights=hl, chromatic_aberration=ca, temporal_denoise=s)
    front = [CR.correct(HR.reconstruct(x, pattern, f32(WB), "rebuild", 0.98, mask), pattern, ca, mask) for x in xs]
    assert (HR.reconstruct(xs[1], pattern, f32(WB), "rebuild", 0.98, mask) > xs[1]).mean() >= 0.02
    assert not np.array_equal(front[1], xs[1])
    ys = T.run(front, s, mask)
    assert_exercised(front[1], ys[0], s, mask, f"{cam} {kind} chain")
    counts = [_count_calls(monkeypatch, e) for e in ("mi_isp_highlights_raw_batch", "mi_isp_chromatic_raw_batch",
                                                     "mi_isp_temporal_raw_batch", "mi_isp_denoise_raw_batch")]
    got = capture(monkeypatch, isp)
    hist = ti.TemporalHistory()
    for k, src in enumerate(srcs):
        got.clear()
        img = call(isp, kind, torch.from_numpy(src).to(dev), defects=m, history=hist).cpu().numpy()
        assert_exact(hist.plane.cpu().numpy(), ys[k], f"{cam} {kind} chain frame {k}: the temporal y")
        cfa = got[0].cpu().numpy()
        D.assert_within_bound(cfa, D.route_yg(ys[k], dn, pixel_gains(grid, H, W), mask), work, f"{cam} {kind} chain {k}",
                              where=~mask)
        assert_exact(cfa, correct_cfa(cfa, mask, work), "defect fix-up")
        check_image(isp, img, cfa, pattern, f"{cam} {kind} chain {k}")
    assert [len(c) for c in counts] == [2, 2, 2, 2]


def test_reset_makes_the_next_frame_a_first_frame(ti, rng, dev, monkeypatch):
    H, W = 66, 70
    s = settings(ti)
    srcs, xs, _, _ = sequence(rng, "p12", H, W, 3)
    isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev, temporal_denoise=s)
    hist = ti.TemporalHistory()
    ts = [torch.from_numpy(f).to(dev) for f in srcs]
    isp.load_packed12(ts[0], history=hist)
    isp.load_packed12(ts[1], history=hist)
    assert hist.frames == 2 and not np.array_equal(hist.plane.cpu().numpy(), xs[1])
    hist.reset()
    assert hist.frames == 0 and hist.plane is None and hist.shape == (H, W)
    isp.load_packed12(ts[2], history=hist)
    assert hist.frames == 1
    assert_exact(hist.plane.cpu().numpy(), xs[2], "the frame after reset()")
    isp.load_packed12(ts[1], history=hist)
    assert_exact(hist.plane.cpu().numpy(), T.blend(xs[1], xs[2], s), "the frame after that")


def test_rejected_calls_leave_the_histories_untouched(ti, rng, dev, monkeypatch):
    H, W = 66, 70
    s = settings(ti)
    srcs, xs, _, _ = sequence(rng, "p12", H, W, 2)
    small = torch.from_numpy(sequence(rng, "p12", 6, 4, 1)[0][0]).to(dev)
    ts = [torch.from_numpy(f).to(dev) for f in srcs]
    on = ti.Camera16(ti.BayerPattern.RGGB, device=dev, temporal_denoise=s)
    off = ti.Camera16(ti.BayerPattern.RGGB, device=dev)
    a, b = ti.TemporalHistory(), ti.TemporalHistory()
    on.load_packed12_batch(ts, history=[a, b])
    before = [h.plane.clone() for h in (a, b)]
    calls = [_count_calls(monkeypatch, e) for e in ENTRIES + ["mi_isp_load_packed_batch_shading", "mi_isp_awb_stats_packed"]]
    for bad, exc in ((lambda: on.load_packed12(ts[0]), ValueError),
                     (lambda: on.load_packed12_batch(ts, history=[a, a]), ValueError),
                     (lambda: on.load_packed12_batch(ts, history=[a]), ValueError),
                     (lambda: on.load_packed12(small, history=a), ValueError),
                     (lambda: off.load_packed12(ts[0], history=a), ValueError),
                     (lambda: off.process_packed12(ts, history=[a, b]), ValueError),
                     (lambda: ti.temporal_cfa(torch.zeros((6, 4), device=dev), a, s), ValueError)):
        with pytest.raises(exc):
            bad()
    # a loader whose stream is being captured into a graph
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    scratch = torch.zeros(8, device=dev)
    with torch.cuda.graph(g, stream=side):
        scratch.add_(1.0)                                     # (the graph is not empty)
        with pytest.raises(RuntimeError, match="graph"):
            on.load_packed12(ts[0], history=a)
        with pytest.raises(RuntimeError, match="graph"):
            on.load_packed12_batch(ts, history=[a, b])
    torch.cuda.synchronize(dev)
    assert sum(len(c) for c in calls) == 0, "a rejected call reached the library"
    for h, p in zip((a, b), before):
        assert h.frames == 1 and h.shape == (H, W)
        assert_exact(h.plane.cpu().numpy(), p.cpu().numpy(), "a rejected call changed a history")
    on.load_packed12(ts[1], history=a)                        # ... and the history still works
    assert_exact(a.plane.cpu().numpy(), T.blend(xs[1], xs[0], s), "the next frame")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_off_calls_no_new_entry_point(ti, rng, dev, monkeypatch, cam, work, kind):
    """An ISP without the stage, and one after set(temporal_denoise=False), reach no mi_isp_temporal_* entry point: with
    chromatic aberration on they make the one chromatic call they made before, and give the same bits."""
    H, W = 66, 70
    srcs, xs, black, white = sequence(rng, kind, H, W, 1, levels=True)
    t = torch.from_numpy(srcs[0]).to(dev)
    ca = ti.ChromaticAberration((1.01, -0.02, 0.005), (0.992, 0.015, 0.0))
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white, lens_shading=make_grid(rng, 5, 7, 4))
    calls = [_count_calls(monkeypatch, e) for e in ENTRIES]
    others = [_count_calls(monkeypatch, e) for e in ("mi_isp_chromatic_raw_batch", "mi_isp_highlights_raw_batch",
                                                     "mi_isp_denoise_raw_batch")]
    for extra, n_ca in ((dict(), 0), (dict(chromatic_aberration=ca), 1)):
        off = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw, **extra)
        on = getattr(ti, cam)(ti.BayerPattern.GBRG, temporal_denoise=settings(ti, kind), **kw, **extra)
        for c in calls + others:
            c.clear()
        a = call(off, kind, t)
        assert sum(len(c) for c in calls) == 0 and [len(c) for c in others] == [n_ca, 0, 0]
        hist = ti.TemporalHistory()
        call(on, kind, t, history=hist)
        assert [len(c) for c in calls] == [0, 1, 0] and hist.frames == 1
        on.set(temporal_denoise=False)
        assert on.temporal_denoise is None
        for c in calls + others:
            c.clear()
        b = call(on, kind, t)
        assert sum(len(c) for c in calls) == 0 and [len(c) for c in others] == [n_ca, 0, 0]
        assert_exact(b.cpu().numpy(), a.cpu().numpy(), f"{cam} {kind} off again")


def test_process_packed12_takes_the_two_calls(ti, rng, dev):
    H, W = 64, 64
    s = settings(ti)
    seqs = [[torch.from_numpy(f).to(dev) for f in sequence(rng, "p12", H, W, 2)[0]] for _ in range(3)]
    kw = dict(device=dev, moving_alpha=0.3, correct_colors=True, temporal_denoise=s)
    a, b = ti.Camera16(ti.BayerPattern.RGGB, **kw), ti.Camera16(ti.BayerPattern.RGGB, **kw)
    ha, hb = [ti.TemporalHistory() for _ in range(3)], [ti.TemporalHistory() for _ in range(3)]
    for step in range(2):
        frames = [q[step] for q in seqs]
        outs, imgs = a.process_packed12(frames, gamma=0.7, keep_images=True, history=ha)
        ref_imgs = b.load_packed12_batch(frames, history=hb)
        ref_outs = b.tonemap_reinhard(ref_imgs, gamma=0.7)
        for o, r in zip(outs, ref_outs):
            assert_exact(o.cpu().numpy(), r.cpu().numpy(), f"step {step} u8")
        for i, r in zip(imgs, ref_imgs):
            assert_exact(i.cpu().numpy(), r.cpu().numpy(), f"step {step} images")
            assert not hasattr(i, "_mi_metering_sub"), "images of a raw route carry no metering subsample"
        for x, y in zip(ha, hb):
            assert x.frames == step + 1
            assert_exact(x.plane.cpu().numpy(), y.plane.cpu().numpy(), f"step {step} history")
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), f"step {step} metering state")
