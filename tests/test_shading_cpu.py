"""Lens shading without a GPU: the Python call surface and the C entry points reject bad grids before any launch, and the
flat-field calibration helper on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

from taichi_image_amd import camera_isp, BayerPattern, Camera16, Camera32


BAD_GRIDS = [
    np.ones((3, 4, 4), np.float32),                # neither one grid nor four
    np.ones((1, 4, 4), np.float32),
    np.ones(16, np.float32),                       # 1-D
    np.ones((1, 5), np.float32),                   # Gh = 1
    np.ones((65, 5), np.float32),                  # Gh = 65
    np.ones((4, 5, 65), np.float32),
    np.full((4, 4), np.nan, np.float32),
    np.where(np.eye(4) > 0, np.inf, 1.0).astype(np.float32),
    -np.ones((4, 4), np.float32),
    np.full((4, 4), 16.5, np.float32),
]


@pytest.mark.parametrize("i", range(len(BAD_GRIDS)))
@pytest.mark.parametrize("cam", [Camera16, Camera32])
def test_bad_grids_raise(cam, i):
    g = BAD_GRIDS[i]
    with pytest.raises(ValueError):
        cam(BayerPattern.RGGB, device=torch.device("cuda", 0), lens_shading=g)
    with pytest.raises(ValueError):
        cam(BayerPattern.RGGB, device=torch.device("cuda", 0), lens_shading=torch.from_numpy(g))
    isp = cam(BayerPattern.RGGB, device=torch.device("cuda", 0))
    with pytest.raises(ValueError):
        isp.set(lens_shading=g)
    assert isp.lens_shading is None


def test_check_shading_accepts():
    g = camera_isp._check_shading(np.ones((2, 64)))
    assert g.shape == (1, 2, 64) and g.dtype == np.float32
    g = camera_isp._check_shading(torch.full((4, 64, 2), 16.0, dtype=torch.float64))
    assert g.shape == (4, 64, 2) and g.max() == 16
    assert camera_isp._check_shading(np.zeros((3, 3))).max() == 0


def test_shading_entry_points_validate_on_the_host():
    from taichi_image_amd import _native
    L = _native.lib()
    assert L.mi_isp_version() >= 1200
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = (ctypes.c_void_p * 1)(p)
    bad = [_native.Shading(p.value, 2, 4, 4), _native.Shading(p.value, 0, 4, 4), _native.Shading(p.value, 4, 1, 4),
           _native.Shading(p.value, 4, 4, 65), _native.Shading(p.value, 1, 65, 2), _native.Shading(None, 4, 4, 4)]
    lv = _native.levels_arg([0, 0, 0, 0], 4095)
    for sh in bad:
        for levels in (None, lv):
            assert L.mi_isp_load_packed_shading(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, levels, sh, None) != 0
            assert b"shading" in L.mi_isp_last_error()
            assert L.mi_isp_load_packed_metered_shading(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, p, 8, levels, sh,
                                                        None) != 0
            assert b"shading" in L.mi_isp_last_error()
            assert L.mi_isp_load_packed_batch_shading(one, one, None, 1, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, 8, levels,
                                                      sh, None) != 0
            assert b"shading" in L.mi_isp_last_error()
        assert L.mi_isp_load_convert_shading(p, p, 4, 8, 0, 2, None, sh, None) != 0
        assert b"shading" in L.mi_isp_last_error()


def radial_gain(H, W, strength=0.3):
    """A radial vignetting gain per site: 1 at the centre, about 1.45 in the corners (a 31 % fall-off)."""
    def g(y, x, s):
        ry, rx = (y - (H - 1) / 2) / (H / 2), (x - (W - 1) / 2) / (W / 2)
        return 1.0 + (strength + 0.05 * s) * (ry * ry + rx * rx) / 2
    return g


def test_calibration_recovers_a_radial_fall_off_on_cpu():
    """Within 2 % of the true gain at the interior nodes.  A border node averages a window the frame clips to its inner
    half, which biases it by the slope of the fall-off there (3 % at most here)."""
    H, W, gh, gw = 768, 1024, 13, 17
    g = radial_gain(H, W)
    rr, cc = np.mgrid[0:H, 0:W].astype(np.float64)
    site = (rr.astype(int) & 1) * 2 + (cc.astype(int) & 1)
    base = np.array([3000.0, 2600.0, 2500.0, 3200.0])
    true = np.stack([g(rr, cc, s) for s in range(4)])
    gain_px = np.choose(site, true)
    black = [64, 66, 65, 64]
    flat = np.round(np.choose(site, base) / gain_px) + np.choose(site, np.array(black, np.float64))
    grid = camera_isp.lens_shading_from_flat(torch.from_numpy(flat.astype(np.int64)), (gh, gw), black_level=black)
    assert isinstance(grid, torch.Tensor) and grid.shape == (4, gh, gw) and grid.dtype == torch.float32
    ys, xs = np.arange(gh) * (H - 1) / (gh - 1), np.arange(gw) * (W - 1) / (gw - 1)
    for s in range(4):
        t = g(ys[:, None], xs[None, :], s)
        expect = t / t.min()                      # max(means) / mean: relative to the brightest (centre) node
        rel = np.abs(grid[s].numpy() / expect - 1)
        assert rel[1:-1, 1:-1].max() < 0.02, (s, rel[1:-1, 1:-1].max())
        assert rel.max() < 0.03, (s, rel.max())
    pooled = camera_isp.lens_shading_from_flat(flat.astype(np.uint16), (gh, gw), black_level=black, per_site=False)
    assert isinstance(pooled, np.ndarray) and pooled.shape == (gh, gw)


def test_calibration_of_a_constant_flat_is_ones():
    flat = np.tile(np.array([[1000, 2000], [1500, 800]], np.uint16), (30, 40))
    grid = camera_isp.lens_shading_from_flat(flat, (5, 7))
    assert grid.shape == (4, 5, 7) and np.all(grid == 1.0)
    grid = camera_isp.lens_shading_from_flat(torch.from_numpy(flat.astype(np.int32)), (2, 2), black_level=[10, 20, 30, 40])
    assert torch.all(grid == 1.0)


def test_calibration_rejects_a_dark_node():
    flat = np.full((40, 60), 500, np.uint16)
    flat[:6, :8] = 0
    with pytest.raises(ValueError):
        camera_isp.lens_shading_from_flat(flat, (5, 5))
    with pytest.raises(ValueError):
        camera_isp.lens_shading_from_flat(np.full((40, 60), 100), (5, 5), black_level=100)
