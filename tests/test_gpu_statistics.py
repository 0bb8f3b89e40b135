"""Frame statistics (Camera16/32 statistics=, statistics_cfa, the C entry points) on the GPU against tests/statistics_ref.py.
Every comparison in this file is the exact equality of all int64 words of a frame's result.

The shapes are the smallest at which the kernel can go wrong, written with the kernel's own geometry (the host-only query
mi_isp_statistics_geometry): frames of one quad, zones of unequal size, zones of one quad (the blocks then add to global
memory directly; the route is asserted from mi_isp_statistics_direct_blocks), one tile plus two pixels, two tiles plus a
remainder with zone borders on a tile seam and inside a tile, and a batch large enough for blocks of two tiles."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import exposure_merge_ref as M
from tests import statistics_ref as R
from tests.test_gpu_denoise import call
from tests.test_gpu_green_equalize import FULL, KINDS, encode, raw_kind
from tests.util import assert_exact

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]
ISP_SHAPE = (66, 70)
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def geometry():
    """(tile rows, tile columns, zone cells of a block's LDS table, the most tiles a block takes)."""
    from taichi_image_amd import _native as N
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib().mi_isp_statistics_geometry(out))
    return tuple(out)


def settings(ti, kind="p12", zones=(3, 5)):
    """The settings in the units of the kind's x (load_16f's x is the code, 0 .. 1000)."""
    scale = 1000.0 if kind == "16f" else 1.0
    return ti.Statistics(zones=zones, clip=0.98 * scale, dark=scale / 64)


def source(rng, kind, H, W, levels=False):
    """(the loader's input, x, black, white) of a generated frame."""
    return encode(kind, R.make_frame(rng, H, W, FULL[kind]), levels)


def same_words(got, want, what):
    got = np.asarray(got).ravel()
    assert got.dtype == np.int64 and got.shape == want.words.shape, what
    bad = np.flatnonzero(got != want.words)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, first at {bad[:8]}: got {got[bad[:8]]}, " \
                          f"want {want.words[bad[:8]]}"


def measure_raw(dev, kind, src, H, W, pattern, s, lv=None, arg=None, garbage=True):
    """mi_isp_statistics_raw on one frame, into a buffer that held garbage."""
    from taichi_image_amd import _native as N
    t = torch.from_numpy(src).to(dev)
    out = torch.full((s.words,), -0x0123456789ABCDEF if garbage else 0, dtype=torch.int64, device=dev)
    N.check(N.lib().mi_isp_statistics_raw(t.data_ptr(), out.data_ptr(), H, W, raw_kind(kind), int(kind == "ids"), pattern, lv,
                                          arg, s._arg(), N.stream_ptr(dev)))
    return out.cpu().numpy()


def direct_blocks(n, H, W, s):
    from taichi_image_amd import _native as N
    return int(N.lib().mi_isp_statistics_direct_blocks(n, H, W, s._arg()))


# ---- statistics_cfa: the shapes ------------------------------------------------------------------------------------------
def test_tiny_frames(ti, rng, dev):
    """2 x 2: one quad, one zone, no focus pixel; 6 x 6: one green pixel per phase whose taps are inside."""
    for (H, W), zones in [((2, 2), (1, 1)), ((6, 6), (1, 1)), ((6, 6), (3, 3)), ((2, 6), (1, 3))]:
        x = (rng.random((H, W)) * 0.9).astype(f32)
        for pattern in PATTERNS:
            s = ti.Statistics(zones=zones)
            q = R.of(s, x, pattern)
            assert int(q.focus[..., 1].sum()) == (2 if (H, W) == (6, 6) else 0)
            got = ti.statistics_cfa(torch.from_numpy(x).to(dev), ti.BayerPattern(pattern), s)
            assert got.buffer.device == dev and got.zones.shape == zones + (4, 4) and got.focus.shape == zones + (2,)
            assert got.histogram.shape == (4, 256)
            same_words(got.buffer.cpu().numpy(), q, f"{H}x{W} zones {zones} p{pattern}")
    host = ti.statistics_cfa(x, ti.BayerPattern.BGGR, s)                       # numpy in: the result is on the device all the same
    same_words(host.buffer.cpu().numpy(), R.of(s, x, O.BGGR), "numpy in")


@pytest.mark.parametrize("zones,direct", [((3, 5), False), ((5, 7), True), ((1, 1), False), ((5, 3), False), ((2, 7), False)])
def test_uneven_zones_and_zones_of_one_quad(ti, rng, dev, geometry, zones, direct):
    """10 x 14: zones of unequal size in the block's LDS table, and one quad per zone - more cells than the table holds, so
    the block adds to global memory directly."""
    H, W = 10, 14
    s = ti.Statistics(zones=zones)
    assert (zones[0] * zones[1] > geometry[2]) == direct and direct_blocks(1, H, W, s) == int(direct)
    for pattern in (O.RGGB, O.GRBG):
        x = (R.make_frame(rng, H, W).astype(f32) * f32(1 / 4095))
        q = R.of(s, x, pattern)
        sizes = {int(n) for n in q.zones[..., 0].sum(axis=2).ravel()}
        assert min(sizes) >= 4 and (zones != (3, 5) or len(sizes) > 1)
        same_words(ti.statistics_cfa(x, ti.BayerPattern(pattern), s).buffer.cpu().numpy(), q, f"zones {zones} p{pattern}")


def test_tile_seams(ti, rng, dev, geometry):
    """One tile plus two pixels on both axes, and two tiles plus a remainder whose zone rows end on the tile seams and
    whose zone columns end inside the tiles; the large zone counts send some blocks to global memory."""
    TH, TW, cells, _ = geometry
    for (H, W), zones in [((TH + 2, TW + 2), (2, 2)), ((TH + 2, TW + 2), (TH // 2, 3)), ((3 * TH - 2, 2 * TW + 6), (3, 4)),
                          ((3 * TH - 2, 2 * TW + 6), (6, 32))]:
        s = ti.Statistics(zones=zones)
        x = (R.make_frame(rng, H, W).astype(f32) * f32(1 / 4095))
        q = R.of(s, x, O.GBRG)
        R.assert_exercised(q, f"{H}x{W}")
        rows = {int(r) for r in np.flatnonzero(np.diff(q.zi[:, 0])) + 1}
        cols = {int(c) for c in np.flatnonzero(np.diff(q.zj[0])) + 1}
        if zones == (3, 4):
            assert rows == {TH, 2 * TH} and cols and all(c % TW for c in cols)
        assert direct_blocks(1, H, W, s) == {(2, 2): 0, (TH // 2, 3): 2, (3, 4): 0, (6, 32): 6}[zones]
        same_words(ti.statistics_cfa(x, ti.BayerPattern.GBRG, s).buffer.cpu().numpy(), q, f"{H}x{W} zones {zones}")


def test_blocks_of_two_tiles(ti, rng, dev, geometry):
    """A batch large enough for every block to take two tiles: a lane then keeps its sums across a tile seam, or adds them
    where its zone column ends there.  32 frames are one source, so there is one reference."""
    from taichi_image_amd import _native as N
    TH, TW, _, _ = geometry
    H, W, n = 4 * TH, 32 * TW, 32
    assert (H // TH) * (W // TW) * n // 2048 == 2
    src, x, _, _ = source(rng, "p12", H, W)
    t = torch.from_numpy(src).to(dev)
    for zones in [(8, 8), (4, 32), (32, 28)]:
        s = ti.Statistics(zones=zones)
        assert (direct_blocks(n, H, W, s) > 0) == (zones == (32, 28))
        q = R.of(s, x, O.RGGB)
        R.assert_exercised(q, f"zones {zones}")
        out = torch.full((n, s.words), 7, dtype=torch.int64, device=dev)
        N.check(N.lib().mi_isp_statistics_raw_batch(
            N.ptr_array([t] * n), N.ptr_array(list(out)), n, H, W, N.MI_RAW_PACKED12, 0, O.RGGB, None, None, s._arg(),
            N.stream_ptr(dev)))
        got = out.cpu().numpy()
        for k in (0, 1, 17, n - 1):
            same_words(got[k], q, f"zones {zones} frame {k}")
        assert (got == got[0]).all()


def test_blocks_of_sixteen_tiles(ti, rng, dev, geometry):
    """The longest strip: 32 launches' worth of tiles, so every block takes MAX_STRIP tiles.  With four zone columns a lane
    keeps its sums over all sixteen tiles - its 10-bit counters at their largest, 128 - and with 32 it adds them every
    other tile.  32 frames are one source, so there is one reference per zone grid."""
    from taichi_image_amd import _native as N
    TH, TW, _, longest = geometry
    H, W, n = 16 * TH, 64 * TW, 32
    assert N.lib().mi_isp_statistics_strip(n, H, W) == longest == 16
    src, x, _, _ = source(rng, "p12", H, W)
    t = torch.from_numpy(src).to(dev)
    for zones in [(4, 4), (32, 32)]:
        s = ti.Statistics(zones=zones)
        q = R.of(s, x, O.GRBG)
        assert direct_blocks(n, H, W, s) == 0
        out = torch.full((n, s.words), -1, dtype=torch.int64, device=dev)
        N.check(N.lib().mi_isp_statistics_raw_batch(
            N.ptr_array([t] * n), N.ptr_array(list(out)), n, H, W, N.MI_RAW_PACKED12, 0, O.GRBG, None, None, s._arg(),
            N.stream_ptr(dev)))
        got = out.cpu().numpy()
        same_words(got[0], q, f"zones {zones} frame 0")
        assert (got == got[0]).all()


# ---- the C entry points: every source kind --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,levels", [(k, lv) for k in KINDS for lv in (False, True) if not lv or k not in ("16f", "32f")])
def test_every_source_kind(ti, rng, dev, kind, levels):
    """mi_isp_statistics_raw on every source kind, packed frames under all four patterns, without and with levels (where
    the kind has them)."""
    H, W = ISP_SHAPE
    packed = kind in ("p12", "ids", "p16")
    s = settings(ti, kind)
    for pattern in PATTERNS if packed else [PATTERNS[KINDS.index(kind) % 4]]:
        src, x, black, white = source(rng, kind, H, W, levels)
        isp = ti.Camera32(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white)
        lv = isp._levels(12 if kind in ("p12", "ids") else 16) if levels else None
        q = R.of(s, x, pattern)
        R.assert_exercised(q, f"{kind} levels={levels}", normalised=kind != "16f")
        same_words(measure_raw(dev, kind, src, H, W, pattern, s, lv), q, f"{kind} p{pattern} levels={levels}")


@pytest.mark.parametrize("work", ["f16", "f32"])
def test_cfa_of_both_dtypes_with_a_defect_map(ti, rng, dev, work):
    H, W = ISP_SHAPE
    x = O.cast_out(R.make_frame(rng, H, W).astype(f32) * f32(1 / 4095), work)
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    s = ti.Statistics(zones=(3, 5))
    for pattern, dm in [(O.RGGB, None), (O.BGGR, m), (O.GRBG, m)]:
        q = R.of(s, x.astype(f32), pattern, None if dm is None else dm.mask())
        R.assert_exercised(q, work)
        got = ti.statistics_cfa(torch.from_numpy(x).to(dev), ti.BayerPattern(pattern), s, defects=dm)
        same_words(got.buffer.cpu().numpy(), q, f"{work} p{pattern} map={dm is not None}")


def defect_sites(H, W):
    """Listed sites that are centres of green pixels, their taps, red and blue sites, corners and tile seams."""
    sites = [(0, 0), (1, 2), (H - 1, W - 1), (H // 2, W // 2), (H // 2 + 1, W // 2), (min(63, H - 1), min(64, W - 1)),
             (min(64, H - 1), min(63, W - 1)), (5, 6), (5, 8), (6, 7), (7, 7), (10, min(40, W - 1)), (20, 21), (22, 21), (20, 23)]
    return sorted(set(sites))


@pytest.mark.parametrize("kind", ["p12", "16u", "32f"])
def test_a_defect_map_whose_sites_are_centres_and_taps(ti, rng, dev, kind):
    H, W = ISP_SHAPE
    pattern = O.GBRG
    s = settings(ti, kind)
    src, x, _, _ = source(rng, kind, H, W)
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    q, plain = R.of(s, x, pattern, m.mask()), R.of(s, x, pattern)
    lost = plain.contributes & ~q.contributes
    assert (lost & m.mask()).any() and (lost & ~m.mask()).any(), "the map has to list centres and taps of focus pixels"
    assert int(q.valid.sum()) == H * W - len(m)
    same_words(measure_raw(dev, kind, src, H, W, pattern, s, None, m._arg(dev)), q, kind)


def test_nan_and_infinities_in_an_f32_source(ti, rng, dev):
    """A NaN and -inf are no pixels (and no taps); +inf is a clipped pixel with v = 65536."""
    H, W = ISP_SHAPE
    x = (R.make_frame(rng, H, W).astype(f32) * f32(1 / 4095))
    spots = defect_sites(H, W)
    for k, (r, c) in enumerate(spots):
        x[r, c] = (np.nan, np.inf, -np.inf)[k % 3]
    x[30, 30:36] = -0.25                                                      # (below zero: v = 0, dark)
    x[31, 30:36] = 1.5                                                        # (above one: v = 65536, clipped)
    s = ti.Statistics(zones=(3, 5))
    q = R.of(s, x, O.RGGB)
    assert int(q.valid.sum()) == H * W - sum(1 for k in range(len(spots)) if k % 3 != 1)
    assert q.histogram[:, 255].sum() >= 6 and q.dark[30, 30:36].all() and q.clipped[31, 30:36].all()
    same_words(measure_raw(dev, "32f", x, H, W, O.RGGB, s), q, "raw 32f")
    same_words(ti.statistics_cfa(x, ti.BayerPattern.RGGB, s).buffer.cpu().numpy(), q, "cfa f32")


def test_a_batch_beyond_one_launch_into_garbage(ti, rng, dev):
    """33 tiny frames through the batch entry point, a map for every other one, into buffers that held garbage: every
    frame's words, the second launch's included."""
    from taichi_image_amd import _native as N
    H, W, n = 6, 10, 33
    s = ti.Statistics(zones=(3, 2), clip=0.7, dark=0.2)
    m = ti.DefectMap([(1, 2), (2, 3), (4, 6)], (H, W))
    xs = [rng.random((H, W)).astype(f32) for _ in range(n)]
    srcs = [torch.from_numpy(x).to(dev) for x in xs]
    out = torch.from_numpy(rng.integers(-2 ** 62, 2 ** 62, (n, s.words))).to(dev)
    arg = m._arg(dev)
    maps = (ctypes.c_void_p * n)(*[ctypes.addressof(arg) if k % 2 else None for k in range(n)])
    N.check(N.lib().mi_isp_statistics_raw_batch(N.ptr_array(srcs), N.ptr_array(list(out)), n, H, W, N.MI_RAW_32F, 0, O.BGGR,
                                                None, maps, s._arg(), N.stream_ptr(dev)))
    got = out.cpu().numpy()
    for k in range(n):
        same_words(got[k], R.of(s, xs[k], O.BGGR, m.mask() if k % 2 else None), f"frame {k}")


def test_the_result_is_cleared_on_every_call(ti, rng, dev):
    """The same buffer twice: the second result does not add to the first."""
    H, W = ISP_SHAPE
    s = ti.Statistics(zones=(2, 2))
    from taichi_image_amd import _native as N
    out = torch.full((s.words,), 2 ** 40 + 3, dtype=torch.int64, device=dev)
    for k in range(2):
        x = (R.make_frame(rng, H, W).astype(f32) * f32(1 / 4095))
        t = torch.from_numpy(x).to(dev)
        N.check(N.lib().mi_isp_statistics_cfa(t.data_ptr(), out.data_ptr(), H, W, N.MI_F32, O.RGGB, None, s._arg(),
                                              N.stream_ptr(dev)))
        same_words(out.cpu().numpy(), R.of(s, x, O.RGGB), f"call {k}")


# ---- through the ISP ---------------------------------------------------------------------------------------------------
def make_isp(ti, dev, cam, pattern, stats, black=None, white=None, stage=False, scale=1.0):
    return getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white,
                            highlights=ti.Highlights(clip=0.9 * scale) if stage else None, statistics=stats)


@pytest.mark.parametrize("stage", [False, True])
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_loader_kind(ti, rng, dev, cam, work, kind, stage):
    """Every loader with levels (where the kind has them) and a defect map, without and with one raw stage on: the image is
    the image of an ISP without the option bit for bit, frame_statistics the reference on the source."""
    H, W = ISP_SHAPE
    pattern = PATTERNS[KINDS.index(kind) % 4]
    s = settings(ti, kind)
    src, x, black, white = source(rng, kind, H, W, levels=True)
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    scale = 1000.0 if kind == "16f" else 1.0
    on = make_isp(ti, dev, cam, pattern, s, black, white, stage, scale)
    off = make_isp(ti, dev, cam, pattern, None, black, white, stage, scale)
    t = torch.from_numpy(src).to(dev)
    img = call(on, kind, t, defects=m)
    assert off.frame_statistics is None and on.statistics is s and off.statistics is None
    assert_exact(img.cpu().numpy(), call(off, kind, t, defects=m).cpu().numpy(), f"{cam} {kind} image")
    assert off.frame_statistics is None and len(on.frame_statistics) == 1
    q = R.of(s, x, pattern, m.mask())
    R.assert_exercised(q, kind, normalised=kind != "16f")
    same_words(on.frame_statistics[0].buffer.cpu().numpy(), q, f"{cam} {kind} stage={stage}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("bits", [12, 16])
def test_the_batch_loaders(ti, rng, dev, cam, work, bits):
    """Three frames, a map for the middle one: one FrameStatistics per frame, new ones on every call."""
    H, W = ISP_SHAPE
    kind = "p12" if bits == 12 else "p16"
    s = settings(ti)
    frames = [source(rng, kind, H, W) for _ in range(3)]
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    maps = [None, m, None]
    on, off = make_isp(ti, dev, cam, O.GRBG, s), make_isp(ti, dev, cam, O.GRBG, None)
    ts = [torch.from_numpy(f[0]).to(dev) for f in frames]
    load = (lambda isp: isp.load_packed12_batch(ts, defects=maps)) if bits == 12 else \
        (lambda isp: isp.load_packed16_batch(ts, defects=maps))
    a, b = load(on), load(off)
    for k in range(3):
        assert_exact(a[k].cpu().numpy(), b[k].cpu().numpy(), f"image {k}")
        same_words(on.frame_statistics[k].buffer.cpu().numpy(),
                   R.of(s, frames[k][1], O.GRBG, None if maps[k] is None else m.mask()), f"{cam} {kind} frame {k}")
    first = on.frame_statistics
    load(on)
    assert len(on.frame_statistics) == 3 and all(p is not r for p, r in zip(first, on.frame_statistics))
    assert on.frame_statistics[0].buffer.data_ptr() != first[0].buffer.data_ptr()


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_a_bracket_loader(ti, rng, dev, cam, work, kind):
    """E = 2: one list per bracket with one entry per exposure, each the reference on that exposure's frame."""
    from tests.test_gpu_exposure_merge import GAIN, RATIOS, READ_NOISE, bracket, load
    H, W = ISP_SHAPE
    merge = ti.ExposureMerge(RATIOS[2], GAIN, READ_NOISE, saturation=0.9)
    s = settings(ti, kind, zones=(2, 3))
    srcs, xs, black, white = bracket(rng, kind, H, W, 2, levels=True)
    m = ti.DefectMap(defect_sites(H, W), (H, W))
    kw = dict(device=dev, black_level=black, white_level=white, exposure_merge=merge)
    on = getattr(ti, cam)(ti.BayerPattern.RGGB, statistics=s, **kw)
    off = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    ts = [torch.from_numpy(f).to(dev) for f in srcs]
    assert_exact(load(on, kind, ts, defects=m).cpu().numpy(), load(off, kind, ts, defects=m).cpu().numpy(), "image")
    assert off.frame_statistics is None and len(on.frame_statistics) == 1 and len(on.frame_statistics[0]) == 2
    for e in range(2):
        same_words(on.frame_statistics[0][e].buffer.cpu().numpy(), R.of(s, xs[e], O.RGGB, m.mask()), f"{kind} exposure {e}")
    if kind == "p12":                                                          # the batch form: two brackets
        on.load_packed12_bracket_batch([ts, ts[::-1]], defects=[m, None])
        assert [len(b) for b in on.frame_statistics] == [2, 2]
        same_words(on.frame_statistics[1][0].buffer.cpu().numpy(), R.of(s, xs[1], O.RGGB), "bracket 1 exposure 0")
        same_words(on.frame_statistics[0][1].buffer.cpu().numpy(), R.of(s, xs[1], O.RGGB, m.mask()), "bracket 0 exposure 1")


@pytest.mark.parametrize("cam,work", CAMS)
def test_process_packed12(ti, rng, dev, cam, work):
    H, W = ISP_SHAPE
    s = settings(ti)
    frames = [source(rng, "p12", H, W) for _ in range(2)]
    ts = [torch.from_numpy(f[0]).to(dev) for f in frames]
    on, off = make_isp(ti, dev, cam, O.BGGR, s), make_isp(ti, dev, cam, O.BGGR, None)
    a, b = on.process_packed12(ts), off.process_packed12(ts)
    for k in range(2):
        assert_exact(a[k].cpu().numpy(), b[k].cpu().numpy(), f"output {k}")
        same_words(on.frame_statistics[k].buffer.cpu().numpy(), R.of(s, frames[k][1], O.BGGR), f"{cam} frame {k}")


@pytest.mark.parametrize("cam,work", CAMS)
def test_a_frame_the_zones_do_not_fit_is_refused_before_anything_runs(ti, rng, dev, monkeypatch, cam, work):
    """Every loader checks the shape rules with its other arguments: a ValueError, no library call, the state as it was."""
    from tests.util import _count_calls
    isp = make_isp(ti, dev, cam, O.RGGB, ti.Statistics(zones=(8, 8)))
    calls = [_count_calls(monkeypatch, name) for name in ("mi_isp_statistics_raw_batch", "mi_isp_load_convert_shading")]
    small = torch.zeros((6, 20), dtype=torch.uint16, device=dev)
    packed = torch.zeros((6, 30), dtype=torch.uint8, device=dev)
    for load in (lambda: isp.load_16u(small), lambda: isp.load_16f(small), lambda: isp.load_32f(small.float()),
                 lambda: isp.load_packed12(packed), lambda: isp.load_packed12_batch([packed, packed]),
                 lambda: isp.process_packed12([packed])):
        with pytest.raises(ValueError, match="statistics: zones 8x8 exceed the 3x10 quads of the frame"):
            load()
    with pytest.raises(ValueError, match="statistics: frames must be even size, got 7x20"):
        isp.load_16u(torch.zeros((7, 20), dtype=torch.uint16, device=dev))
    assert all(len(c) == 0 for c in calls) and isp.frame_statistics is None and isp.metrics is None


def test_option_off(ti, rng, dev):
    """set(statistics=None) turns the option off: frame_statistics is None again, and stays so; set() without the argument
    leaves the option as it is."""
    H, W = ISP_SHAPE
    s = settings(ti)
    src, x, _, _ = source(rng, "p12", H, W)
    t = torch.from_numpy(src).to(dev)
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev)
    isp.load_packed12(t)
    assert isp.frame_statistics is None
    isp.set(statistics=s)
    isp.load_packed12(t)
    same_words(isp.frame_statistics[0].buffer.cpu().numpy(), R.of(s, x, O.RGGB), "set on")
    isp.set(moving_alpha=0.5)
    assert isp.statistics is s
    isp.set(statistics=None)
    assert isp.frame_statistics is None and isp.statistics is None
    isp.load_packed12(t)
    assert isp.frame_statistics is None
    isp.set(statistics=s)
    isp.set(statistics=False)
    assert isp.statistics is None
    with pytest.raises(ValueError, match="statistics must be None or a Statistics"):
        isp.set(statistics=(8, 8))


def test_the_helpers(ti, rng, dev):
    """mean, clipped_fraction, dark_fraction, sharpness and percentile against the same f64 expressions on the
    reference's integers; a zone without a pixel of a site, or without a focus pixel, is NaN."""
    H, W = ISP_SHAPE
    s = ti.Statistics(zones=(3, 5))
    x = (R.make_frame(rng, H, W).astype(f32) * f32(1 / 4095))
    x[:22, :14][1::2, 1::2] = np.nan                                          # zone (0, 0) has no pixel of site 3 ...
    x[:22, 56:] = 1.0                                                         # ... and zone (0, 4) no focus pixel
    q = R.of(s, x, O.RGGB)
    assert q.zones[0, 0, 3, 0] == 0 and q.focus[0, 4, 1] == 0
    got = ti.statistics_cfa(x, ti.BayerPattern.RGGB, s)
    same_words(got.buffer.cpu().numpy(), q, "words")
    for name in ("mean", "clipped_fraction", "dark_fraction", "sharpness"):
        a, b = getattr(got, name)(), getattr(R, name)(q)
        assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name
    assert np.isnan(got.mean()[0, 0, 3]) and np.isnan(got.sharpness()[0, 4]) and np.isfinite(got.sharpness()[1, 1])
    for p in (0, 1, 50, 99, 100):
        for site in (None, 0, 1, 2, 3):
            assert got.percentile(p, site) == R.percentile(q, p, site), (p, site)
    assert got.percentile(1) < got.percentile(50) < got.percentile(99)
    with pytest.raises(ValueError, match="q must be"):
        got.percentile(101)
    with pytest.raises(ValueError, match="site must be"):
        got.percentile(50, 4)
