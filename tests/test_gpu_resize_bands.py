"""The fused resize loaders (ISP.load_packed12 with resize_width / scale) on frames wider than one source band.

rstrm::resize_kernel (csrc/isp_stream_resize.h) splits a frame into source column bands of at most 62 eight-pixel units,
one wave per band and per rows_per_wave rows, and most of its hard logic sits at the band seams: destination columns
dealt to bands by their quad origin, seams moved up to a multiple of four destination columns (align4) with up to three
pixels borrowed from the right neighbour, the band's last lane taking its right halo from an edge dword, a second
column-group loop for bands that produce more than 256 destination columns, and one source row demosaiced past the rows
a wave owns.  Frames of at most 512 columns run all of that with ONE band; this file pins it on two and three bands
(520 / 528 / 1008 / 1016 columns), on the tall frame that raises rows_per_wave, and - through the C ABI - at scales below
the range the Python layer sends.

Every comparison is bit for bit against oracle.isp_oracle.isp_load_packed12 (with levels or shading:
tests.test_gpu_shading.ref_load).  The oracle's full-resolution image of a frame is computed once and shared by the
scales that resize it (isp_load_packed12 is exactly demosaic-then-resize_bilinear).
"""
import math

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests.test_gpu_levels_matrix import DARK, LEVELS
from tests.test_gpu_shading import make_grid, ref_load
from tests.util import assert_exact, natural_packed12

gpu = pytest.mark.gpu
f32 = np.float32



@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]
H_SMALL = 38                                        # ten row bands of rows_per_wave 4, the last one 2 rows
BAND_WIDTHS = [520, 528, 1008, 1016]                # see test_geometry_of_the_cases
TILE_WIDTH = 1018                                   # W % 8 != 0: the resize tile kernel on both work types
TALL = (4100, 520)
# a resize_width with Wd % 4 == 2 (element stores at the seams) whose scale the Python layer still sends fused
RW_MOD4_2 = {520: 210, 528: 210, 1008: 398, 1016: 406, 1018: 406}
# scale classes: name -> the camera's resize argument for a frame of width W
SCALE_CLASSES = {
    "config3": lambda W: dict(scale=0.46875),
    "0.8": lambda W: dict(scale=0.8),
    "wd_mod4_2": lambda W: dict(resize_width=RW_MOD4_2[W]),
    "1.0": lambda W: dict(scale=1.0),
    "1.3": lambda W: dict(scale=1.3),
    "2.5": lambda W: dict(scale=2.5),
}
SUB_RANGE_SCALES = [0.3, 0.2, 0.1]                  # below mi_isp_load_packed_scale_supported: the C ABI only
# 38 x 584 at 0.1: the raw seam is destination column 29 (29 % 4 == 1), so a kernel that kept align4 on there would
# borrow three pixels whose quads reach 23 source columns past the band - more than the two extra units (16) hold
SUB_RANGE_FRAMES = [(38, 1016), (64, 520), (38, 584)]


# ---- rstrm::geometry and rtile::scales_fit, restated -------------------------------------------------------------------
# Carried over BY HAND from rstrm::geometry / rstrm::first_with_origin / the kernel's band_edge
# (taichi_image_amd/csrc/isp_stream_resize.h) and rtile::scales_fit (taichi_image_amd/csrc/isp_resize_tile.h): a change
# there must be repeated here, and the cases below re-read against it.
def geometry(H, W, scale):
    units = W // 8
    bands_x = (units - 2 + 61) // 62 if units > 2 else 1
    stride_units = (units - 2 + bands_x - 1) // bands_x if units > 2 else 1
    step = math.ceil(f32(1.0) / f32(scale))
    rpw = (H * bands_x + 2047) // 2048
    rpw = max((rpw + 1) // 2 * 2, 4)
    return dict(units=units, bands_x=bands_x, stride_units=stride_units,
                last_band_units=units - (bands_x - 1) * stride_units, align4=int(3 * step + 2 <= 16),
                rows_per_wave=rpw, bands_y=(H + rpw - 1) // rpw, last_band_rows=H - (H - 1) // rpw * rpw)


def scales_fit(s0, s1):
    s0, s1 = f32(s0), f32(s1)
    rows = int(f32(15) / s0) + 1 + 6 + 1
    cols = int(f32(63) / s1) + 1 + 6 + 1 + 7
    return bool(s0 > 0 and s1 > 0 and rows <= 48 and cols <= 176)


def _quad_origin(i, s, n):
    return min(int(f32(i) / s), n - 2)


def _first_with_origin(x, s, n_src, n_dst):
    c = max(int(f32(x) * s) - 2, 0)
    while c < n_dst and _quad_origin(c, s, n_src) < x:
        c += 1
    return min(c, n_dst)


def band_columns(W, Wd, scale):
    """[cd_begin, cd_end) of every band: the destination columns its wave produces."""
    g, s = geometry(2, W, scale), f32(scale)

    def edge(src_col):
        c = _first_with_origin(src_col, s, W, Wd)
        return min((c + 3) & ~3 if g["align4"] else c, Wd)
    starts = [0] + [edge(b * g["stride_units"] * 8) for b in range(1, g["bands_x"])]
    return list(zip(starts, starts[1:] + [Wd]))


def _kw_scale(H, W, kw):
    """((Wd, Hd), scale) of a camera's resize argument, as the oracle sizes it."""
    return O.isp_output_size(H, W, kw.get("resize_width", 0), kw.get("scale"))


def test_geometry_of_the_cases():
    """What the GPU cases below assume about rstrm::geometry, stated: each frame size is in the list for one property."""
    g = {W: geometry(H_SMALL, W, 0.8) for W in BAND_WIDTHS + [512]}
    assert g[512]["bands_x"] == 1 and g[520]["bands_x"] == 2                      # the narrowest two-band frame
    assert (g[520]["units"], g[520]["stride_units"], g[520]["last_band_units"]) == (65, 32, 33)  # last band: stride + 1
    assert (g[528]["units"], g[528]["bands_x"], g[528]["stride_units"], g[528]["last_band_units"]) == (66, 2, 32, 34)
    assert g[528]["last_band_units"] == g[528]["stride_units"] + 2               # both extra lanes own a unit
    assert (g[1008]["units"], g[1008]["bands_x"], g[1008]["stride_units"], g[1008]["last_band_units"]) == (126, 2, 62, 64)
    assert (g[1016]["units"], g[1016]["bands_x"], g[1016]["stride_units"], g[1016]["last_band_units"]) == (127, 3, 42, 43)
    for W in BAND_WIDTHS:                            # every wave fits the 64 lanes; H = 38: ten row bands, the last 2 rows
        assert g[W]["last_band_units"] <= 64 and g[W]["stride_units"] + 2 <= 64
        assert (g[W]["rows_per_wave"], g[W]["bands_y"], g[W]["last_band_rows"]) == (4, 10, 2)
    assert TILE_WIDTH % 8 != 0 and TILE_WIDTH % 2 == 0                            # not a streaming width
    t = geometry(*TALL, 0.8)
    assert (t["bands_x"], t["rows_per_wave"], t["bands_y"], t["last_band_rows"]) == (2, 6, 684, 2)
    for H, W in SUB_RANGE_FRAMES:
        assert geometry(H, W, 0.3)["bands_x"] > 1 and geometry(H, W, 0.3)["rows_per_wave"] == 4

    # the second column-group loop: more than 256 destination columns from one band
    for scale, per_band in ((1.3, 437), (2.5, 840)):
        (Wd, _), _ = _kw_scale(H_SMALL, 1016, dict(scale=scale))
        widths = [e - b for b, e in band_columns(1016, Wd, scale)]                # 42, 42 and 43 units' worth
        assert min(widths) > 256 and all(abs(w - per_band) <= 4 for w in widths[:-1]), (scale, widths)
    # ... on every width at 1.3 and 2.5, at 0.8 on the bands of 1008 and 1016 (42 units and more: a downscale with a
    # second group), and never at the two smallest scales
    for W in BAND_WIDTHS:
        for name, over in (("2.5", True), ("1.3", True), ("0.8", W >= 1008), ("config3", False), ("wd_mod4_2", False)):
            (Wd, _), s = _kw_scale(H_SMALL, W, SCALE_CLASSES[name](W))
            assert (max(e - b for b, e in band_columns(W, Wd, s)) > 256) == over, (W, name)
    # the seams are where align4 put them: a multiple of 4, and for some case moved (the borrowed pixels exist)
    moved = 0
    for W in BAND_WIDTHS:
        for name in SCALE_CLASSES:
            (Wd, _), s = _kw_scale(H_SMALL, W, SCALE_CLASSES[name](W))
            bands = band_columns(W, Wd, s)
            assert bands[0][0] == 0 and bands[-1][1] == Wd and all(b < e for b, e in bands)
            assert all(b % 4 == 0 for b, _ in bands)
            g_w = geometry(H_SMALL, W, s)
            raw = [_first_with_origin(k * g_w["stride_units"] * 8, f32(s), W, Wd) for k in range(1, g_w["bands_x"])]
            moved += sum(r % 4 != 0 for r in raw)
    assert moved > 0

    # the element-store class: Wd % 4 == 2 and still a scale the Python layer sends to the fused kernels
    for W, rw in RW_MOD4_2.items():
        assert rw % 4 == 2 and scales_fit(rw / W, rw / W), (W, rw)
    # every scale sent through Python passes scales_fit (the loaders stay fused); align4 holds for all of them
    for W in BAND_WIDTHS + [TILE_WIDTH]:
        for name in SCALE_CLASSES:
            _, s = _kw_scale(H_SMALL, W, SCALE_CLASSES[name](W))
            assert scales_fit(s, s) and geometry(H_SMALL, W, s)["align4"] == 1, (W, name)
    assert scales_fit(0.8, 0.8)                      # the tall frame, the unaligned output
    # below the range: 0.3 skips source rows (< 1/3) with align4 still on; 0.2 and 0.1 switch align4 off
    assert [scales_fit(s, s) for s in SUB_RANGE_SCALES] == [False, False, False]
    assert [geometry(38, 1016, s)["align4"] for s in SUB_RANGE_SCALES] == [1, 0, 0]
    assert all(s < 1 / 3 for s in SUB_RANGE_SCALES)
    # why align4 has to end: had the seams been moved up at these scales too, the quad of the last borrowed pixel would
    # end `reach` source columns past the band's own ones; the wave demosaics 16.  Some case must exceed that, or a
    # kernel with align4 stuck on computes the same image everywhere (at 1016 and 520 the reach stays below 16).
    reach = {}
    for H, W in SUB_RANGE_FRAMES:
        for scale in SUB_RANGE_SCALES:
            (Wd, _), s = _kw_scale(H, W, dict(scale=scale))
            g_w = geometry(H, W, s)
            for k in range(1, g_w["bands_x"]):
                x = k * g_w["stride_units"] * 8
                c = _first_with_origin(x, f32(s), W, Wd)
                c4 = min((c + 3) & ~3, Wd)
                if c4 > c:
                    reach[W, scale] = max(reach.get((W, scale), 0), _quad_origin(c4 - 1, f32(s), W) + 2 - x)
    assert reach[584, 0.1] == 24 and geometry(38, 584, 0.1)["align4"] == 0
    assert all(r <= 16 for (W, _), r in reach.items() if W != 584)


def test_scales_fit_is_the_library_s():
    """The restated admission test against mi_isp_load_packed_scale_supported (a host function: no GPU needed)."""
    from taichi_image_amd import _native
    L = _native.lib()
    scales = [0.1, 0.2, 0.25, 0.3, 1 / 3, 0.375, 0.38, 0.3888, 0.389, 0.39, 0.3996, 0.46875, 0.8, 1.0, 1.3, 2.5]
    scales += [rw / W for W, rw in RW_MOD4_2.items()]
    for s in scales:
        assert bool(L.mi_isp_load_packed_scale_supported(float(s))) == scales_fit(s, s), s


# ---- references --------------------------------------------------------------------------------------------------------
_FULL = {}


def _shared(key, make):
    """A full-resolution oracle image, computed once per frame and settings and left read-only."""
    if key not in _FULL:
        a = make()
        a.setflags(write=False)
        _FULL[key] = a
    return _FULL[key]


def _full_plain(packed, work, pattern, cc):
    ccm = O.isp_color_matrix(cc, O.DEFAULT_WB, O.DEFAULT_CC)
    return _shared((hash(packed.tobytes()), work, pattern, cc), lambda: O.isp_load_packed12(packed, work, pattern, correct_colors=ccm))


def _resized(full, kw):
    """O.isp_load_packed12's resize step (oracle/isp_oracle.py: isp_output_size, then resize_bilinear)."""
    sz = _kw_scale(full.shape[0], full.shape[1], kw)
    return O.resize_bilinear(full, sz[0], sz[1])


def _dev(dev, packed):
    return torch.from_numpy(packed).to(dev)


def _cc(*idx):
    """correct_colors on for half of the cases, spread so that every scale class has it on some pattern."""
    return sum(idx) % 2 == 0


# ---- 2. seams, column groups and stores --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("scale_class", list(SCALE_CLASSES))
@pytest.mark.parametrize("W", BAND_WIDTHS + [TILE_WIDTH])
def test_resize_across_bands(ti, rng, dev, cam, work, pattern, scale_class, W):
    """Every width x scale class x pattern on both work types (Camera16: the stream resize kernel, and the resize tile
    kernel at W = 1018; Camera32: the resize tile kernel), with the colour matrix on half of them."""
    H = H_SMALL
    kw = SCALE_CLASSES[scale_class](W)
    cc = _cc(pattern, list(SCALE_CLASSES).index(scale_class), W // 8)
    packed = natural_packed12(rng, H, W, pattern)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=cc, **kw)
    src = _dev(dev, packed)
    got = isp.load_packed12(src).cpu().numpy()
    full = _full_plain(packed, work, pattern, cc)
    want = _resized(full, kw)
    what = f"{cam} {H}x{W} p{pattern} {kw} cc={cc}"
    assert_exact(got, want, what)
    if scale_class == "1.0":                         # a resize by 1 is the plain load
        assert_exact(got, full, what + " against the plain load")


def test_colour_matrix_meets_every_scale_class():
    """The spread of _cc: on Camera16 every scale class has correct_colors on and off on some pattern, at every width."""
    for W in BAND_WIDTHS + [TILE_WIDTH]:
        for i in range(len(SCALE_CLASSES)):
            assert {_cc(p, i, W // 8) for p in PATTERNS} == {True, False}


@gpu
@pytest.mark.parametrize("pattern", [O.GRBG, O.BGGR])
def test_metering_subsample_of_a_wide_resized_load(ti, rng, dev, pattern):
    """The stride-8 metering subsample of a three-band resized load is ref[::8, ::8], bit for bit.  ISP.load_packed12 tags
    a subsample (_mi_metering_sub) only on full-resolution loads - a resized image carries none, which
    test_gpu_parity.test_load_packed_leaves_the_metering_subsample asserts - so the subsample of the resized load is taken
    where the library offers it: mi_isp_load_packed_metered, the gather behind the stream resize kernel."""
    from taichi_image_amd import _native
    H, W, scale = H_SMALL, 1016, 0.46875
    packed = natural_packed12(rng, H, W, pattern)
    want = _resized(_full_plain(packed, "f16", pattern, False), dict(scale=scale))
    Hd, Wd = want.shape[:2]
    src = _dev(dev, packed)
    img = ti.Camera16(ti.BayerPattern(pattern), device=dev, scale=scale).load_packed12(src)
    assert_exact(img.cpu().numpy(), want, "the resized load")
    assert getattr(img, "_mi_metering_sub", None) is None
    rgb = torch.empty((Hd, Wd, 3), dtype=torch.float16, device=dev)
    sub = torch.full(((Hd + 7) // 8, (Wd + 7) // 8, 3), -1.0, dtype=torch.float16, device=dev)
    _native.check(_native.lib().mi_isp_load_packed_metered(src.data_ptr(), rgb.data_ptr(), H, W, 12, 0, pattern, None,
                                                           _native.MI_F16, Hd, Wd, scale, sub.data_ptr(), 8,
                                                           _native.stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    assert_exact(rgb.cpu().numpy(), want, "mi_isp_load_packed_metered: image")
    assert_exact(sub.cpu().numpy(), want[::8, ::8], "mi_isp_load_packed_metered: subsample")


# ---- 3. levels and shading instances on three bands --------------------------------------------------------------------
def _levels_case(rng, pattern, case, n_frames=1):
    """Frames, the grid (or None) and the levels of one LEVELS case at 38 x 1016."""
    black, white, sites = LEVELS[case]
    frames = [natural_packed12(rng, H_SMALL, 1016, pattern, dark=DARK if n_frames == 1 else 0.02 * k)
              for k in range(n_frames)]
    grid = None if sites is None else make_grid(rng, 17, 13, sites)
    return frames, grid, black, white


def _full_levels(packed, work, pattern, case, grid, black, white):
    key = (hash(packed.tobytes()), work, pattern, case, None if grid is None else hash(grid.tobytes()))
    return _shared(key, lambda: ref_load(packed, 12, work, pattern, grid, black, white))


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("scale", [0.46875, 1.3])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", list(LEVELS))
def test_levels_and_shading_on_three_bands(ti, rng, dev, cam, work, scale, pattern, case):
    """The levels / shading instances of the resize kernels (LV 0-3 per pattern) where a band's col0 is not 0: the
    per-wave shading node row and the per-site levels on the middle and the last band."""
    (packed,), grid, black, white = _levels_case(rng, pattern, case)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white,
                           lens_shading=grid, scale=scale)
    src = _dev(dev, packed)
    got = isp.load_packed12(src).cpu().numpy()
    want = _resized(_full_levels(packed, work, pattern, case, grid, black, white), dict(scale=scale))
    assert_exact(got, want, f"{cam} p{pattern} {case} scale {scale}")


@gpu
@pytest.mark.parametrize("pattern,case,scale", [(p, c, s) for p, c, s in zip(PATTERNS, LEVELS, (0.46875, 1.3, 0.46875, 1.3))])
def test_batch_of_ten_on_three_bands(ti, rng, dev, pattern, case, scale):
    """load_packed12_batch of 10 frames (two launches, grid.y = 8 and 2) on three bands, one levels case per pattern;
    every frame against its own reference."""
    frames, grid, black, white = _levels_case(rng, pattern, case, n_frames=10)
    isp = ti.Camera16(ti.BayerPattern(pattern), device=dev, black_level=black, white_level=white, lens_shading=grid,
                      scale=scale)
    srcs = [_dev(dev, f) for f in frames]
    got = isp.load_packed12_batch(srcs)
    assert len(got) == 10
    for k, (g, f) in enumerate(zip(got, frames)):
        want = _resized(ref_load(f, 12, "f16", pattern, grid, black, white), dict(scale=scale))
        assert_exact(g.cpu().numpy(), want, f"p{pattern} {case} scale {scale} frame {k}")


# ---- 4. rows per wave above 4 ------------------------------------------------------------------------------------------
@gpu
def test_rows_per_wave_six(ti, rng, dev):
    """4100 x 520: two bands and 684 row bands of rows_per_wave 6, the last one 2 rows; GBRG with the colour matrix."""
    from oracle import c_oracle
    H, W = TALL
    packed = natural_packed12(rng, H, W, O.GBRG)
    isp = ti.Camera16(ti.BayerPattern.GBRG, device=dev, correct_colors=True, scale=0.8)
    src = _dev(dev, packed)
    got = isp.load_packed12(src).cpu().numpy()
    ccm = O.isp_color_matrix(True, O.DEFAULT_WB, O.DEFAULT_CC)
    if c_oracle.available():      # the demosaic from the C oracle (fast), the resize from the NumPy oracle
        cfa = c_oracle.decode12_scaled(packed, work="f16").reshape(H, W)
        rgb = c_oracle.demosaic(cfa, O.GBRG, ccm=ccm, round_f16=True).astype(np.float16)
    else:
        rgb = O.bayer_to_rgb(O.decode12(packed, "f16", scaled=True), O.GBRG, ccm)
    assert_exact(got, _resized(rgb, dict(scale=0.8)), "4100x520 GBRG scale 0.8")


# ---- 5. the C ABI below the Python layer's scale range -----------------------------------------------------------------
def _c_load(dev, packed, out, H, W, pattern, cc, work_code, Hd, Wd, scale):
    from taichi_image_amd import _native
    ccm = _native.ccm_arg(O.isp_color_matrix(cc, O.DEFAULT_WB, O.DEFAULT_CC))
    src = _dev(dev, packed)                          # alive until the launch has finished
    rc = _native.lib().mi_isp_load_packed(src.data_ptr(), out.data_ptr(), H, W, 12, 0, pattern, ccm, work_code, Hd, Wd,
                                          float(scale), _native.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("scale", SUB_RANGE_SCALES)
@pytest.mark.parametrize("shape", SUB_RANGE_FRAMES)
def test_c_abi_f16_takes_any_positive_scale(ti, rng, dev, shape, scale, pattern):
    """mi_isp_load_packed with MI_F16 on a frame the streaming kernel takes, at scales the Python layer never sends
    (include/mi_isp.h: any positive scale): row skipping below 1/3, align4 off below 1/4.  The same call with MI_F32 is
    refused and writes nothing."""
    from taichi_image_amd import _native
    H, W = shape
    cc = _cc(pattern, SUB_RANGE_SCALES.index(scale))
    packed = natural_packed12(rng, H, W, pattern)
    want = _resized(_full_plain(packed, "f16", pattern, cc), dict(scale=scale))
    Hd, Wd = want.shape[:2]
    out = torch.full((Hd, Wd, 3), -1.0, dtype=torch.float16, device=dev)
    assert _c_load(dev, packed, out, H, W, pattern, cc, _native.MI_F16, Hd, Wd, scale) == 0
    assert_exact(out.cpu().numpy(), want, f"MI_F16 {H}x{W} p{pattern} scale {scale} cc={cc}")
    out32 = torch.full((Hd, Wd, 3), -1.0, dtype=torch.float32, device=dev)
    assert _c_load(dev, packed, out32, H, W, pattern, cc, _native.MI_F32, Hd, Wd, scale) != 0
    assert bool((out32 == -1.0).all()), "the refused MI_F32 call wrote to its output"


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SUB_RANGE_FRAMES)
def test_c_abi_f16_output_off_its_8_byte_boundary(ti, rng, dev, shape, pattern):
    """An MI_F16 output one f16 element off its allocation (not 8-byte aligned) is not the streaming kernel's: the call
    falls to the resize tile kernel and gives the same bits; the element before the image stays untouched."""
    from taichi_image_amd import _native
    H, W = shape
    scale, cc = 0.8, _cc(pattern)
    packed = natural_packed12(rng, H, W, pattern)
    want = _resized(_full_plain(packed, "f16", pattern, cc), dict(scale=scale))
    Hd, Wd = want.shape[:2]
    buf = torch.full((Hd * Wd * 3 + 1,), -1.0, dtype=torch.float16, device=dev)
    out = buf[1:].view(Hd, Wd, 3)
    assert out.data_ptr() % 8 == 2 and out.is_contiguous()
    assert _c_load(dev, packed, out, H, W, pattern, cc, _native.MI_F16, Hd, Wd, scale) == 0
    assert_exact(out.cpu().numpy(), want, f"unaligned MI_F16 {H}x{W} p{pattern}")
    assert float(buf[0]) == -1.0
