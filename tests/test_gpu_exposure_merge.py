"""Exposure merge (Camera16/32 exposure_merge= and the bracket loaders, merge_cfa, the three C entries) on the GPU against
tests/exposure_merge_ref.py.

The route's CFA is captured by wrapping ISP._process_image; it must equal the NumPy f32 contract bit for bit (with the
defect fix-up of tests/test_defects_cpu.py at listed sites), and the loader's image must be O.bayer_to_rgb /
O.resize_bilinear of that CFA bit for bit.  The tile is 64 x 64 and the halo 2: the shapes are the smallest that reach
every seam.  The brackets (exposure_merge_ref.make_bracket) put every class of pixel in a frame, which the reference alone
asserts."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chromatic_ref as CR
from tests import denoise_ref as D
from tests import exposure_merge_ref as M
from tests import highlights_ref as HR
from tests import temporal_ref as T
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_denoise import call, capture, loader_x
from tests.test_gpu_shading import make_grid, pixel_gains
from tests.test_gpu_temporal import cfa_of, check_image, encode, seam_defects
from tests.util import _count_calls, assert_exact

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
CCM = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
WB = np.array([1.8, 1.0, 2.1])
SHAPES = [(2, 2), (2, 4), (6, 4), (64, 64), (66, 70), (130, 66)]
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]
ENTRIES = ["mi_isp_merge_raw", "mi_isp_merge_raw_batch", "mi_isp_merge_cfa"]
RATIOS = {2: (1, 4), 3: (1, 4, 16), 4: (1, 2, 4, 8)}
GAIN, READ_NOISE = 2.4e-4, 1.5e-3
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def settings(ti, E, kind="p12", **kw):
    """The noise model and the saturation of the generated brackets in the units of the kind's x (load_16f's x is the
    code, 0 .. 1000)."""
    scale = 1000.0 if kind == "16f" else 1.0
    return ti.ExposureMerge(RATIOS[E], GAIN * scale, READ_NOISE * scale, saturation=0.9 * scale, **kw)


def bracket(rng, kind, H, W, E, levels=False):
    """One bracket: ([the loader's inputs], [their x], black, white)."""
    out = [encode(kind, u, levels) for u in M.make_bracket(rng, H, W, RATIOS[E], GAIN, READ_NOISE)]
    return [o[0] for o in out], [o[1] for o in out], out[0][2], out[0][3]


def load(isp, kind, ts, **kw):
    """The bracket loader of the kind."""
    if kind == "p16":
        return isp.load_packed16_bracket(ts, **kw)
    if kind in ("p12", "ids"):
        return isp.load_packed12_bracket(ts, ids_format=kind == "ids", **kw)
    return {"16u": isp.load_16u_bracket, "16f": isp.load_16f_bracket, "32f": isp.load_32f_bracket}[kind](ts, **kw)


def assert_exercised(xs, s, mask, what):
    """On the reference alone: a bracket of 4096 pixels or more has 10 % of its pixels in each of the four classes."""
    if xs[0].size >= 4096:
        shares = M.classes(xs, s, mask)
        assert min(shares) >= 0.10, f"{what}: the bracket does not exercise the operator {shares}"


def to_dev(srcs, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in srcs]


# ---- merge_cfa ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
def test_merge_cfa(ti, rng, dev, work):
    for i, (H, W) in enumerate(SHAPES + [(1, 5), (3, 1), (65, 67)]):
        E = 2 + i % 3
        s = settings(ti, E)
        xs = [O.cast_out(u.astype(f32), work) for u in M.make_bracket(rng, H, W, RATIOS[E], GAIN, READ_NOISE)]
        x32 = [x.astype(f32) for x in xs]
        assert_exercised(x32, s, None, f"{work} {H}x{W}")
        want = O.cast_out(M.merge(x32, s), work)
        got = ti.merge_cfa(to_dev(xs, dev), s)
        assert got.device == dev and got.shape == (H, W)
        assert_exact(got.cpu().numpy(), want, f"{work} {H}x{W} E={E}")
        host = ti.merge_cfa(xs, s)                                             # numpy in, numpy out
        assert isinstance(host, np.ndarray)
        assert_exact(host, want, "numpy round trip")
    empty = ti.merge_cfa([np.zeros((0, 8), f32)] * 2, settings(ti, 2))
    assert empty.shape == (0, 8)


@pytest.mark.parametrize("H,W", [(66, 70), (130, 66)])
def test_every_rounding_and_the_orders(ti, rng, dev, H, W):
    """A bracket whose weights are almost all partial: y follows every rounding of the metric and of the weighted sums, the
    order of the taps and of the exposures included (tests/test_exposure_merge_cpu.py shows that each reversed order
    changes more than 5 % of this bracket).  Through merge_cfa, and through load_32f_bracket with a defect map."""
    frames, args = M.rounding_bracket(rng, H, W)
    s = ti.ExposureMerge(*args)
    y = M.merge(frames, s)
    assert (y != M.merge(frames, s, taps=M.TAPS[::-1])).mean() > 0.05
    assert (y != M.merge(frames, s, order=[2, 1])).mean() > 0.05
    ts = to_dev(frames, dev)
    assert_exact(ti.merge_cfa(ts, s).cpu().numpy(), y, f"{H}x{W} merge_cfa")
    m = seam_defects(ti, rng, H, W)
    isp = ti.Camera32(ti.BayerPattern.RGGB, device=dev, exposure_merge=s)
    with pytest.MonkeyPatch.context() as mp:
        got = capture(mp, isp)
        isp.load_32f_bracket(ts, defects=m)
        assert_exact(got[0].cpu().numpy(), correct_cfa(M.merge(frames, s, m.mask()), m.mask(), "f32"), f"{H}x{W} with a map")


# ---- the loaders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", [2, 3, 4])
def test_every_source_kind_and_shape(ti, rng, dev, monkeypatch, cam, work, kind, E):
    """Every source kind, both work dtypes and every E at every shape; levels and a per-site grid at the seam shapes.  The
    kinds that take an odd-sized frame get one through mi_isp_merge_raw (the demosaic behind the loaders takes even sizes
    only)."""
    s = settings(ti, E, kind)
    if kind in ("16u", "16f", "32f"):
        from taichi_image_amd import _native
        H, W = 67, 69
        srcs, xs, _, _ = bracket(rng, kind, H, W, E)
        assert_exercised(xs, s, None, f"{kind} E={E} {H}x{W}")
        out = torch.empty((H, W), dtype=torch.float16 if work == "f16" else torch.float32, device=dev)
        mode = {"16u": _native.MI_RAW_16U, "16f": _native.MI_RAW_16F, "32f": _native.MI_RAW_32F}[kind]
        _native.check(_native.lib().mi_isp_merge_raw(
            _native.ptr_array(to_dev(srcs, dev)), out.data_ptr(), H, W, mode, 0,
            _native.MI_F16 if work == "f16" else _native.MI_F32, None, None, None, s._arg(), 0, _native.stream_ptr(dev)))
        assert_exact(out.cpu().numpy(), O.cast_out(M.merge(xs, s), work), f"{cam} {kind} E={E} {H}x{W}")
    for i, (H, W) in enumerate(SHAPES):
        pattern = (i + E) % 4
        extras = H * W >= 4096 and (i & 1) == 0
        srcs, xs, black, white = bracket(rng, kind, H, W, E, levels=extras)
        grid = make_grid(rng, 5, 7, 4) if extras else None
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, color_correction=CCM,
                               black_level=black, white_level=white, lens_shading=grid, exposure_merge=s)
        got = capture(monkeypatch, isp)
        what = f"{cam} {kind} E={E} p{pattern} {H}x{W} extras={extras}"
        assert_exercised(xs, s, None, what)
        y = M.merge(xs, s)
        img = load(isp, kind, to_dev(srcs, dev)).cpu().numpy()
        want = cfa_of(isp, y, work)
        assert len(got) == 1
        assert_exact(got[0].cpu().numpy(), want, what + " CFA")
        check_image(isp, img, want, pattern, what)
        got.clear()


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_levels_awb_gains_a_grid_and_a_defect_map(ti, rng, dev, monkeypatch, cam, work, kind):
    """AWB on (the effective grid E is the gain, the statistics read frame 0 of the bracket), levels, and a defect map with
    listed centres and listed taps on both sides of the tile seams: a listed site never feeds a neighbour's metric and is
    itself replaced by the fix-up."""
    H, W = 66, 70
    pattern = O.GBRG
    s = settings(ti, 3, kind)
    m = seam_defects(ti, rng, H, W)
    mask = m.mask()
    kw = dict(device=dev, correct_colors=True, auto_white_balance=True, moving_alpha=0.5, lens_shading=make_grid(rng, 5, 7, 4))
    srcs, xs, black, white = bracket(rng, kind, H, W, 3, levels=True)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), exposure_merge=s, black_level=black, white_level=white, **kw)
    plain = getattr(ti, cam)(ti.BayerPattern(pattern), black_level=black, white_level=white, **kw)
    ts = to_dev(srcs, dev)
    load(isp, kind, ts, defects=m)
    call(plain, kind, ts[0], defects=m)
    assert_exact(isp._awb_pending.cpu().numpy(), plain._awb_pending.cpu().numpy(), "pending statistics: frame 0's")
    isp.update_white_balance()
    assert not np.array_equal(isp._awb_gains.cpu().numpy(), f32(WB)), "the update left the seed"
    got = capture(monkeypatch, isp)
    img = load(isp, kind, ts, defects=m).cpu().numpy()
    y = M.merge(xs, s, mask)
    assert_exercised(xs, s, mask, f"{cam} {kind}")
    assert not np.array_equal(y, M.merge(xs, s)), "the map changes no weight: the case shows nothing"
    want = cfa_of(isp, y, work, mask)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} {kind} awb + defects CFA")
    check_image(isp, img, want, pattern, f"{cam} {kind} awb + defects")


# ---- the C entries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
def test_c_entries_single_batch_and_plain(ti, rng, dev, work):
    """mi_isp_merge_raw in the CFA form and the plain form; a batch of three brackets in one launch, one of them with a
    defect map, equals three single calls; mi_isp_merge_cfa."""
    from taichi_image_amd import _native
    L, stream = _native.lib(), _native.stream_ptr(dev)
    H, W, E = 66, 70, 3
    s = settings(ti, E)
    code = _native.MI_F16 if work == "f16" else _native.MI_F32
    tdt = torch.float16 if work == "f16" else torch.float32
    m = seam_defects(ti, rng, H, W)
    mask, arg = m.mask(), m._arg(dev)
    hosts = [[u.astype(f32) for u in M.make_bracket(rng, H, W, RATIOS[E], GAIN, READ_NOISE)] for _ in range(3)]
    maps = [None, arg, None]
    wants = [M.merge(b, s, mask if k == 1 else None) for k, b in enumerate(hosts)]
    assert_exercised(hosts[1], s, mask, "C entries")
    devs = [to_dev(b, dev) for b in hosts]
    new = lambda dt=torch.float32: torch.empty((H, W), dtype=dt, device=dev)  # noqa: E731
    singles = []
    for k in range(3):
        cfa, yp = new(tdt), new()
        _native.check(L.mi_isp_merge_raw(_native.ptr_array(devs[k]), cfa.data_ptr(), H, W, _native.MI_RAW_32F, 0, code, None,
                                         None, maps[k], s._arg(), 0, stream))
        _native.check(L.mi_isp_merge_raw(_native.ptr_array(devs[k]), yp.data_ptr(), H, W, _native.MI_RAW_32F, 0, code, None,
                                         None, maps[k], s._arg(), 1, stream))
        assert_exact(yp.cpu().numpy(), wants[k], f"single {k} plain y")
        assert_exact(cfa.cpu().numpy(), O.cast_out(wants[k], work), f"single {k} CFA")
        singles.append(cfa)
    # one launch: the pointers bracket-major, one map per bracket
    cfas, ys = [new(tdt) for _ in range(3)], [new() for _ in range(3)]
    flat = _native.ptr_array([f for b in devs for f in b])
    p_maps = (ctypes.c_void_p * 3)(None, ctypes.addressof(arg), None)
    _native.check(L.mi_isp_merge_raw_batch(flat, _native.ptr_array(cfas), 3, H, W, _native.MI_RAW_32F, 0, code, None, None,
                                           p_maps, s._arg(), 0, stream))
    _native.check(L.mi_isp_merge_raw_batch(flat, _native.ptr_array(ys), 3, H, W, _native.MI_RAW_32F, 0, code, None, None,
                                           p_maps, s._arg(), 1, stream))
    for k in range(3):
        assert_exact(cfas[k].cpu().numpy(), singles[k].cpu().numpy(), f"batch {k} CFA")
        assert_exact(ys[k].cpu().numpy(), wants[k], f"batch {k} plain y")
    # mi_isp_merge_cfa
    xs = [O.cast_out(x, work) for x in hosts[0]]
    out = new(tdt)
    _native.check(L.mi_isp_merge_cfa(_native.ptr_array(to_dev(xs, dev)), out.data_ptr(), H, W, code, s._arg(), stream))
    assert_exact(out.cpu().numpy(), O.cast_out(M.merge([x.astype(f32) for x in xs], s), work), "merge_cfa")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("bits", [12, 16])
def test_batch_loaders_equal_single_bracket_loads(ti, rng, dev, monkeypatch, cam, work, bits):
    """Three cameras' brackets in one load_packed*_bracket_batch call, one of them with a defect map, give the bits of three
    single bracket loads, in ONE launch of the stage."""
    H, W, E = 66, 70, 3
    kind = "p12" if bits == 12 else "p16"
    s = settings(ti, E)
    kw = dict(device=dev, correct_colors=True, lens_shading=make_grid(rng, 3, 4, 1), exposure_merge=s)
    a = getattr(ti, cam)(ti.BayerPattern.GRBG, **kw)
    b = getattr(ti, cam)(ti.BayerPattern.GRBG, **kw)
    m = seam_defects(ti, rng, H, W)
    brackets = [to_dev(bracket(rng, kind, H, W, E)[0], dev) for _ in range(3)]
    maps = [None, m, None]
    load_a = a.load_packed12_bracket_batch if bits == 12 else a.load_packed16_bracket_batch
    load_b = b.load_packed12_bracket if bits == 12 else b.load_packed16_bracket
    n = _count_calls(monkeypatch, "mi_isp_merge_raw_batch")
    imgs = load_a(brackets, defects=maps)
    assert len(n) == 1
    for k in range(3):
        ref = load_b(brackets[k], defects=maps[k])
        assert_exact(imgs[k].cpu().numpy(), ref.cpu().numpy(), f"{cam} {bits} camera {k} image")
        assert not hasattr(imgs[k], "_mi_metering_sub"), "images of a raw route carry no metering subsample"
    assert not torch.equal(imgs[0], imgs[2])


# ---- exact properties, chains, state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_saturated_long_frames_equal_the_plain_load_of_frame_0(ti, rng, dev, cam, work, kind):
    """Long frames at or above the saturation everywhere: the bracket load gives the bits of the plain load of frame 0 -
    levels, shading, AWB, defects and the resize included."""
    H, W, E = 66, 70, 3
    levels = kind in ("p12", "ids", "p16", "16u")
    us = M.make_bracket(rng, H, W, RATIOS[E], GAIN, READ_NOISE)
    us = [us[0]] + [0.95 + 0.05 * rng.random((H, W)) for _ in range(E - 1)]
    enc = [encode(kind, u, levels) for u in us]
    srcs, xs, black, white = [o[0] for o in enc], [o[1] for o in enc], enc[0][2], enc[0][3]
    s = settings(ti, E, kind)
    assert all(np.all(x >= f32(s.saturation)) for x in xs[1:])
    m = seam_defects(ti, rng, H, W)
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white, auto_white_balance=True,
              lens_shading=make_grid(rng, 5, 7, 4), resize_width=36)
    on = getattr(ti, cam)(ti.BayerPattern.GBRG, exposure_merge=s, **kw)
    off = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw)
    ts = to_dev(srcs, dev)
    a = load(on, kind, ts, defects=m)
    b = call(off, kind, ts[0], defects=m)
    assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"{cam} {kind}")
    assert_exact(on._awb_pending.cpu().numpy(), off._awb_pending.cpu().numpy(), "pending statistics")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_chain_of_all_five_raw_stages(ti, rng, dev, monkeypatch, cam, work, kind):
    """Exposure merge -> highlights -> chromatic aberration -> temporal -> raw denoise over two brackets of one camera: the
    references applied in that order.  The temporal stage's y (the history) is bit-exact, so the merged y it was fed is;
    the final CFA holds the denoise filter's own bound (tests/denoise_ref.py) against the NumPy chain."""
    H, W, E = 66, 70, 3
    pattern = O.GRBG
    full = {"p12": 4095, "16u": 65535}[kind]
    s = settings(ti, E)
    tn = ti.TemporalDenoise(GAIN, READ_NOISE)
    dn = ti.RawDenoise(0.002, 0.01, strength=1.5, radius=1)
    hl = ti.Highlights("rebuild", 0.98)
    ca = ti.ChromaticAberration((1.01, -0.02, 0.005), (0.992, 0.015, 0.0))
    m = ti.DefectMap([(0, 0), (30, 31), (63, 64), (65, 69), (33, 0), (60, 62), (62, 66), (64, 58)], (H, W))
    mask = m.mask()
    grid = make_grid(rng, 5, 7, 4)
    blobs = HR.make_codes(rng, H, W, full, int(0.985 * full) + 1, pattern) >= int(0.985 * full) + 1
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, lens_shading=grid, raw_denoise=dn,
                           highlights=hl, chromatic_aberration=ca, temporal_denoise=tn, exposure_merge=s)
    all_srcs, merged = [], []
    for _ in range(2):
        srcs, xs = [], []
        for u in M.make_bracket(rng, H, W, RATIOS[E], GAIN, READ_NOISE):     # clipped blobs in every frame of the bracket
            codes = np.where(blobs, full, np.rint(u * full)).astype(np.uint16)
            srcs.append(O.encode12(codes) if kind == "p12" else codes)
            xs.append(loader_x(kind, codes, None, None))
        all_srcs.append(srcs)
        y = M.merge(xs, s, mask)
        assert np.array_equal(y[blobs], xs[0][blobs]) and np.all(y[blobs] == 1)   # clipping still reads as clipping
        assert min(M.classes(xs, s, mask)) >= 0.05           # (the blobs take their share of every class of make_bracket)
        merged.append(y)
    front = [CR.correct(HR.reconstruct(y, pattern, f32(WB), "rebuild", 0.98, mask), pattern, ca, mask) for y in merged]
    assert (HR.reconstruct(merged[1], pattern, f32(WB), "rebuild", 0.98, mask) > merged[1]).mean() >= 0.02
    ys = T.run(front, tn, mask)
    counts = [_count_calls(monkeypatch, e) for e in ("mi_isp_merge_raw_batch", "mi_isp_highlights_raw_batch",
                                                     "mi_isp_chromatic_raw_batch", "mi_isp_temporal_raw_batch",
                                                     "mi_isp_denoise_raw_batch")]
    got = capture(monkeypatch, isp)
    hist = ti.TemporalHistory()
    for k, srcs in enumerate(all_srcs):
        got.clear()
        img = load(isp, kind, to_dev(srcs, dev), defects=m, history=hist).cpu().numpy()
        assert_exact(hist.plane.cpu().numpy(), ys[k], f"{cam} {kind} chain bracket {k}: the temporal y")
        cfa = got[0].cpu().numpy()
        D.assert_within_bound(cfa, D.route_yg(ys[k], dn, pixel_gains(grid, H, W), mask), work, f"{cam} {kind} chain {k}",
                              where=~mask)
        assert_exact(cfa, correct_cfa(cfa, mask, work), "defect fix-up")
        check_image(isp, img, cfa, pattern, f"{cam} {kind} chain {k}")
    assert [len(c) for c in counts] == [2, 2, 2, 2, 2]


@pytest.mark.parametrize("kind", ["p12", "32f"])
def test_merge_then_temporal_the_history_holds_the_merged_y(ti, rng, dev, monkeypatch, kind):
    """Merge -> temporal over three brackets of one camera: the history plane is the temporal blend of the merged frames,
    and the CFA its gained cast."""
    H, W, E = 66, 70, 2
    s = settings(ti, E)
    tn = ti.TemporalDenoise(GAIN, READ_NOISE)
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, exposure_merge=s, temporal_denoise=tn,
                      lens_shading=make_grid(rng, 3, 4, 1))
    got = capture(monkeypatch, isp)
    hist = ti.TemporalHistory()
    h = None
    base = M.make_bracket(rng, H, W, RATIOS[E], GAIN, READ_NOISE)
    for k in range(3):
        us = [np.clip(u + rng.normal(0, 1, u.shape) * M.noise_sigma(u, GAIN, READ_NOISE), 0, 1) for u in base]
        enc = [encode(kind, u) for u in us]
        y = M.merge([o[1] for o in enc], s)
        h = T.blend(y, h, tn)
        got.clear()
        load(isp, kind, to_dev([o[0] for o in enc], dev), history=hist)
        assert hist.frames == k + 1
        assert_exact(hist.plane.cpu().numpy(), h, f"{kind} bracket {k} history")
        assert_exact(got[0].cpu().numpy(), cfa_of(isp, h, "f16"), f"{kind} bracket {k} CFA")
        if k:
            assert not np.array_equal(h, y), "the history did not matter"


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_off_calls_no_new_entry_point(ti, rng, dev, monkeypatch, cam, work, kind):
    """An ISP without the stage, and one after set(exposure_merge=False), reach no mi_isp_merge_* entry point and give
    the same bits."""
    H, W, E = 66, 70, 2
    srcs, xs, black, white = bracket(rng, kind, H, W, E, levels=True)
    ts = to_dev(srcs, dev)
    kw = dict(device=dev, correct_colors=True, black_level=black, white_level=white, lens_shading=make_grid(rng, 5, 7, 4))
    calls = [_count_calls(monkeypatch, e) for e in ENTRIES]
    for extra in (dict(), dict(highlights=ti.Highlights("rebuild", 0.98))):
        off = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw, **extra)
        on = getattr(ti, cam)(ti.BayerPattern.GBRG, exposure_merge=settings(ti, E, kind), **kw, **extra)
        for c in calls:
            c.clear()
        a = call(off, kind, ts[0])
        assert sum(len(c) for c in calls) == 0
        load(on, kind, ts)
        assert [len(c) for c in calls] == [0, 1, 0]
        on.set(exposure_merge=False)
        assert on.exposure_merge is None
        for c in calls:
            c.clear()
        b = call(on, kind, ts[0])
        assert sum(len(c) for c in calls) == 0
        assert_exact(b.cpu().numpy(), a.cpu().numpy(), f"{cam} {kind} off again")


def test_a_bracket_loader_captured_into_a_graph(ti, rng, dev):
    """The stage has no state: a bracket loader captured into a graph and replayed once gives the same image."""
    H, W, E = 66, 70, 3
    s = settings(ti, E)
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, exposure_merge=s,
                      lens_shading=make_grid(rng, 3, 4, 1))
    srcs = bracket(rng, "p12", H, W, E)[0]
    ts = to_dev(srcs, dev)
    ref = isp.load_packed12_bracket(ts).clone()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        img = isp.load_packed12_bracket(ts)
    img.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert_exact(img.cpu().numpy(), ref.cpu().numpy(), "the replayed bracket load")
