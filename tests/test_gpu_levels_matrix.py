"""Sensor levels and lens shading on every CFA pattern: each pattern's instantiations of the loaders (stream, tile, stream
resize, resize tile, metering subsample), of the camera-group kernel and of the sharded camera group, against the oracle.

The levels and shading kernels are compiled once per pattern (isp_*_inst.inc), so a mistake in one pattern's instance - a
swapped site, a wrong row parity - shows only on that pattern.  test_gpu_levels.py / test_gpu_shading.py go deep on one or
two patterns; this file goes wide: all four, small frames, every route.  Expected values: tests/test_gpu_shading.py's
reference (the levels and shading contract of DESIGN.md 3 in NumPy f32, then the oracle's demosaic / resize / tonemap).
"""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests.test_gpu_shading import make_grid, pixel_gains, ref_load, site_levels
from tests.util import _count_calls, assert_close, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]
PER_SITE = [64, 200, 180, 256]
# (black, white, grid sites): levels mode 1 (uniform black), 2 (per site), shading without levels, shading with levels
LEVELS = {"uniform": (300, None, None), "per_site": (PER_SITE, 3900, None), "grid1": (None, None, 1),
          "grid4_per_site": (PER_SITE, 3900, 4)}
DARK = 0.08                                         # (some codes fall below the black levels: the clamp at 0 is exercised)
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _dev(dev, packed):
    return torch.from_numpy(packed).to(dev)


def _check_sub(img, ref, what):
    """The metering subsample the streaming load tagged on the image, bit for bit against ref[::8, ::8]."""
    sub = getattr(img, "_mi_metering_sub", None)
    assert sub is not None and sub[1] == 8, f"{what}: no stride-8 metering subsample tagged"
    assert_exact(sub[0].cpu().numpy(), ref[::8, ::8], f"{what}: metering subsample")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", list(LEVELS))
def test_loader_matrix(ti, rng, dev, cam, work, pattern, case):
    """One pattern and one levels / shading mode through every loader route, bit for bit."""
    black, white, sites = LEVELS[case]
    grid = None if sites is None else make_grid(rng, 17, 13, sites)

    def camera(**kw):
        return getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white,
                                lens_shading=grid, **kw)

    def ref(p, rw=0):
        return ref_load(p, 12, work, pattern, grid, black, white, resize_width=rw)

    what = f"{cam} p{pattern} {case}"
    isp = camera()
    # full resolution: the streaming kernel (with the metering subsample on the way) and the tile kernel (ragged width)
    for (H, W) in ((64, 256), (34, 130)):
        packed = natural_packed12(rng, H, W, pattern, dark=DARK)
        img = isp.load_packed12(_dev(dev, packed))
        want = ref(packed)
        assert_exact(img.cpu().numpy(), want, f"{what} {H}x{W}")
        if W % 8 == 0:
            _check_sub(img, want, f"{what} {H}x{W}")
    # fused resize (the stream resize kernel on Camera16, the resize tile kernel on Camera32) at two scales, and a ragged
    # width with a resize (the resize tile kernel on both work types)
    for (H, W), rw in (((96, 256), 128), ((96, 256), 200), ((34, 130), 64)):
        packed = natural_packed12(rng, H, W, pattern, dark=DARK)
        got = camera(resize_width=rw).load_packed12(_dev(dev, packed)).cpu().numpy()
        assert_exact(got, ref(packed, rw), f"{what} {H}x{W} resize_width {rw}")
    # a batch of 10 frames: two launches of at most 8 cameras, at full resolution (subsamples on the way) and resized
    for (H, W), rw in (((64, 256), 0), ((96, 256), 128)):
        frames = [natural_packed12(rng, H, W, pattern, dark=0.02 * k) for k in range(10)]
        got = camera(resize_width=rw).load_packed12_batch([_dev(dev, f) for f in frames])
        assert len(got) == 10
        for k, (g, f) in enumerate(zip(got, frames)):
            want = ref(f, rw)
            assert_exact(g.cpu().numpy(), want, f"{what} batch {H}x{W} resize_width {rw} frame {k}")
            if rw == 0:
                _check_sub(g, want, f"{what} batch frame {k}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("sites", [None, 4])
def test_colour_matrix_with_levels(ti, rng, dev, cam, work, sites):
    """correct_colors=True with per-site levels (and a 4-site grid): the matrix after the levels and the gain, on the
    stream, tile, fused-resize and batch loaders and load_16u."""
    grid = None if sites is None else make_grid(rng, 17, 13, sites)
    for pattern in PATTERNS:
        def camera(**kw):
            return getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, black_level=PER_SITE,
                                    white_level=3900, lens_shading=grid, **kw)
        isp = camera()
        ccm = isp.color_correct_matrix
        assert ccm is not None
        what = f"{cam} p{pattern} grid {sites}"
        for (H, W) in ((64, 256), (34, 130)):
            packed = natural_packed12(rng, H, W, pattern, dark=DARK)
            img = isp.load_packed12(_dev(dev, packed))
            want = ref_load(packed, 12, work, pattern, grid, PER_SITE, 3900, ccm=ccm)
            assert_exact(img.cpu().numpy(), want, f"{what} {H}x{W}")
            if W % 8 == 0:
                _check_sub(img, want, f"{what} {H}x{W}")
        packed = natural_packed12(rng, 96, 256, pattern, dark=DARK)
        got = camera(resize_width=128).load_packed12(_dev(dev, packed)).cpu().numpy()
        assert_exact(got, ref_load(packed, 12, work, pattern, grid, PER_SITE, 3900, resize_width=128, ccm=ccm),
                     f"{what} resize")
        frames = [natural_packed12(rng, 64, 256, pattern, dark=0.03 * k) for k in range(9)]
        for k, (g, f) in enumerate(zip(isp.load_packed12_batch([_dev(dev, f) for f in frames]), frames)):
            assert_exact(g.cpu().numpy(), ref_load(f, 12, work, pattern, grid, PER_SITE, 3900, ccm=ccm), f"{what} batch {k}")
        # load_16u: its own division, cast(f32(max(v - b_s, 0)) / f32(white - b_s) * gain), then demosaic + matrix
        H, W = 34, 130
        u16 = rng.integers(0, 65536, (H, W), dtype=np.uint16)
        isp.set(white_level=60000)
        x = np.maximum(u16.astype(np.int64) - site_levels(PER_SITE, H, W), 0).astype(f32) / \
            (60000 - site_levels(PER_SITE, H, W)).astype(f32)
        if grid is not None:
            x = x * pixel_gains(grid, H, W)
        got = isp.load_16u(_dev(dev, u16)).cpu().numpy()
        assert_exact(got, O.bayer_to_rgb(O.cast_out(x, work), pattern, correct_colors=ccm), f"{what} load_16u")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("black,white", [(300, None), (PER_SITE, 3900)])
def test_ids_layout_with_levels(ti, rng, dev, cam, work, black, white):
    """The IDS byte layout with levels and no grid (the tile kernel's general fill, levels only), every pattern."""
    for (H, W) in ((64, 256), (34, 130)):
        for pattern in PATTERNS:
            ids = natural_packed12(rng, H, W, pattern, ids_format=True, dark=DARK)
            isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white)
            got = isp.load_packed12(_dev(dev, ids), ids_format=True).cpu().numpy()
            assert_exact(got, ref_load(ids, 12, work, pattern, None, black, white, ids_format=True),
                         f"{cam} IDS {H}x{W} p{pattern} {black}/{white}")


# the shapes, patterns, tonemap arguments and colour matrix of test_gpu_parity.py's
# test_isp_process_packed12_equals_the_two_calls: rows that do not fill a wave's 12, bands narrower than 512 columns
GROUP_CASES = [
    ((48, 64), 3, "RGGB", dict(), False), ((36, 520), 2, "GRBG", dict(gamma=0.6), True),
    ((100, 1032), 4, "BGGR", dict(gamma=0.6, color_adapt=0.3, intensity=1.2, light_adapt=0.7), True),
    ((768, 1024), 6, "GBRG", dict(gamma=2.2), False), ((26, 4096), 2, "RGGB", dict(gamma=0.6), False)]
GROUP_LEVELS = [(300, None), (PER_SITE, 3900)]      # levels mode 1 and 2 of the camera-group kernel


@pytest.mark.parametrize("shape,n,pattern,kw,cc", GROUP_CASES)
@pytest.mark.parametrize("black,white", GROUP_LEVELS)
def test_camera_group_levels_equals_the_two_calls(ti, dev, monkeypatch, shape, n, pattern, kw, cc, black, white):
    """process_packed12 with levels on the camera-group kernel (checked: it fits and the call reaches
    mi_isp_camera_group_reinhard_levels) gives the u8 outputs, the images and the metering state of load_packed12_batch +
    tonemap_reinhard with the same levels, bit for bit, over three groups of a rolling metering; on (36, 520) also the
    oracle chain within the parity tolerances."""
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = shape
    pat = getattr(ti.BayerPattern, pattern)
    lv = _native.levels_arg(*ti.camera_isp._check_levels(black, white, 12))
    assert L.mi_isp_camera_group_fits_levels(H, W, pat.value, ti.types.f16.code, 8, lv) == 1
    kwc = dict(moving_alpha=0.3, correct_colors=cc, device=dev, black_level=black, white_level=white)
    a, b = ti.Camera16(pat, **kwc), ti.Camera16(pat, **kwc)
    fused = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard_levels")
    oracle = shape == (36, 520)
    st = O.IspState(0.3)
    for group in range(3):
        packs = [natural_packed12(np.random.default_rng(1500 + 10 * group + k), H, W, pat.value, dark=0.03 * k + 0.02)
                 for k in range(n)]
        frames = [_dev(dev, p) for p in packs]
        keep = group != 1                                 # (the bench's form - nothing kept - in the middle group)
        got = a.process_packed12(frames, keep_images=keep, **kw)
        assert len(fused) == group + 1, "process_packed12 with levels did not take the camera-group kernel"
        outs, images = got if keep else (got, None)
        want_images = b.load_packed12_batch(frames)
        want = b.tonemap_reinhard(want_images, **kw)
        torch.cuda.synchronize()
        assert L.mi_isp_camera_group_faults(0) == 0
        assert torch.equal(a.metrics.view(torch.int32), b.metrics.view(torch.int32)), f"group {group}: metering state"
        for k in range(n):
            assert torch.equal(outs[k], want[k]), f"group {group} camera {k}: u8 output"
            if keep:
                assert torch.equal(images[k].view(torch.int16), want_images[k].view(torch.int16)), f"group {group} camera {k}: p"
        if oracle:
            refs = [ref_load(p, 12, "f16", pat.value, None, black, white, ccm=a.color_correct_matrix) for p in packs]
            m = st.update_metering(refs)
            assert_close(a.metrics.cpu().numpy(), m, f"group {group}: metrics vs oracle", rel=2e-5)
            for k in range(n):
                ref_u8, ref_p = O.reinhard_isp(refs[k], m, **kw)
                assert_close(outs[k].cpu().numpy(), ref_u8, f"group {group} camera {k}: u8 vs oracle")
                if keep:
                    assert_close(images[k].cpu().numpy(), ref_p, f"group {group} camera {k}: p vs oracle")


@pytest.mark.parametrize("pattern", ["GRBG", "GBRG"])
@pytest.mark.parametrize("black,white", GROUP_LEVELS)
def test_sharded_camera_group_levels(ti, dev, monkeypatch, pattern, black, white):
    """The sharded camera group (subsample with levels -> the sharded metering -> tonemap with levels) on one rank: a
    process_group that is not initialised gives world size 1 but the three-step path.  The same metering state and outputs
    as the unsharded camera-group call, over three steps."""
    H, W, n = 100, 1032, 3
    pat = getattr(ti.BayerPattern, pattern)
    kwc = dict(moving_alpha=0.3, device=dev, black_level=black, white_level=white)
    a = ti.Camera16(pat, **kwc)
    b = ti.Camera16(pat, process_group=object(), **kwc)          # one "rank"
    fused = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard_levels")
    sub = _count_calls(monkeypatch, "mi_isp_camera_group_subsample_levels")
    tonemap = _count_calls(monkeypatch, "mi_isp_camera_group_tonemap_levels")
    for step in range(3):
        frames = [_dev(dev, natural_packed12(np.random.default_rng(1600 + 10 * step + k), H, W, pat.value,
                                             dark=0.02 + 0.03 * k)) for k in range(n)]
        oa = a.process_packed12(frames, gamma=0.6)
        ob = b.process_packed12(frames, gamma=0.6)
        assert len(sub) == step + 1 and len(tonemap) == step + 1, "the sharded camera group was not taken"
        assert_close(b.metrics.cpu().numpy(), a.metrics.cpu().numpy(), f"metering state, step {step}", rel=1e-5)
        for k, (x, y) in enumerate(zip(oa, ob)):
            assert_close(y.cpu().numpy(), x.cpu().numpy(), f"u8 output {k}, step {step}")
    assert len(fused) == 3, "the unsharded camera did not take the camera-group kernel"
    from taichi_image_amd import _native
    assert _native.lib().mi_isp_camera_group_faults(0) == 0


def test_shading_grid_update_between_graph_replays(ti, rng, dev):
    """set(lens_shading=...) and a captured load_packed12: a grid of the same shape is copied in place, so the next replay
    reads the new gains; a grid of another shape is a new tensor, and the graph keeps reading the retired one."""
    H, W = 64, 256
    pattern = O.GBRG
    packed = natural_packed12(rng, H, W, pattern, dark=DARK)
    d = _dev(dev, packed)
    g1, g2, g3 = make_grid(rng, 17, 13, 4), make_grid(rng, 17, 13, 4), make_grid(rng, 9, 5, 4)
    isp = ti.Camera16(ti.BayerPattern(pattern), device=dev, black_level=PER_SITE, white_level=3900, lens_shading=g1)

    def ref(grid):
        return ref_load(packed, 12, "f16", pattern, grid, PER_SITE, 3900)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        isp.load_packed12(d)                                     # warm, outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            out = isp.load_packed12(d)
    torch.cuda.current_stream(dev).wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert_exact(out.cpu().numpy(), ref(g1), "first replay")
    isp.set(lens_shading=g2)                                     # same shape: in place, on the current stream
    graph.replay()
    torch.cuda.synchronize()
    assert_exact(out.cpu().numpy(), ref(g2), "replay after a same-shape grid")
    isp.set(lens_shading=g3)                                     # another shape: a new tensor; g2's stays alive
    graph.replay()
    torch.cuda.synchronize()
    assert_exact(out.cpu().numpy(), ref(g2), "replay after a grid of another shape")
    assert_exact(isp.load_packed12(d).cpu().numpy(), ref(g3), "an eager load after the new shape")


@pytest.mark.parametrize("black,white", [(None, None), (PER_SITE, 3900)])
def test_process_packed12_inside_a_capture_takes_the_two_calls(ti, dev, monkeypatch, black, white):
    """Captured, process_packed12 takes load_packed12_batch + tonemap_reinhard (no camera-group launch goes into a graph),
    with and without levels; the replay gives the eager two calls' outputs and metering state, bit for bit."""
    H, W, n = 36, 520, 2
    kwc = dict(moving_alpha=0.3, device=dev, black_level=black, white_level=white)
    a, b, warm = (ti.Camera16(ti.BayerPattern.GRBG, **kwc) for _ in range(3))
    groups = [[_dev(dev, natural_packed12(np.random.default_rng(1700 + 10 * g + k), H, W, O.GRBG, dark=0.03 * k + 0.02))
               for k in range(n)] for g in range(2)]
    name = "mi_isp_camera_group_reinhard" if black is None else "mi_isp_camera_group_reinhard_levels"
    fused = _count_calls(monkeypatch, name)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        a.process_packed12(groups[0], gamma=0.6)                 # eager: the camera-group kernel
        warm.tonemap_reinhard(warm.load_packed12_batch(groups[0]), gamma=0.6)   # the two calls' workspace, on s
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s):
            outs, images = a.process_packed12(groups[1], gamma=0.6, keep_images=True)
    assert len(fused) == 1, "a camera-group launch went into the capture"
    torch.cuda.current_stream(dev).wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    b.process_packed12(groups[0], gamma=0.6)
    want_images = b.load_packed12_batch(groups[1])
    want = b.tonemap_reinhard(want_images, gamma=0.6)
    torch.cuda.synchronize()
    assert torch.equal(a.metrics.view(torch.int32), b.metrics.view(torch.int32)), "metering state"
    for k in range(n):
        assert torch.equal(outs[k], want[k]), f"camera {k}: u8 output"
        assert torch.equal(images[k].view(torch.int16), want_images[k].view(torch.int16)), f"camera {k}: p"
