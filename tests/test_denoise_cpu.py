"""Raw noise reduction without a GPU: the NumPy statement of the contract (tests/denoise_ref.py) and its properties,
noise_model_from_frames on synthetic frames, and the settings' checks in Python and in the C entry points."""
import ctypes
import math

import numpy as np
import pytest

from oracle import isp_oracle as O
from taichi_image_amd import camera_isp
from taichi_image_amd.denoise import RawDenoise, check_raw_denoise, noise_model_from_frames
from tests import denoise_ref as D

f32 = np.float32
GAIN, READ = 0.002, 0.006                     # a 12-bit sensor's noise model in units of the white level


def poisson_gaussian(rng, x, gain=GAIN, read=READ):
    """x plus zero-mean noise of variance gain * x + read**2."""
    return x + rng.normal(0.0, 1.0, x.shape) * np.sqrt(gain * x + read * read)


# ---- reference properties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
def test_constant_frames_come_back_unchanged(radius):
    """A constant frame, and a frame with a different constant per CFA site: the sites never mix."""
    dn = RawDenoise(GAIN, READ, radius=radius)
    x = np.full((18, 22), 0.3)
    np.testing.assert_allclose(D.filter_x(x, dn), x, rtol=1e-13, atol=0)
    sites = np.empty((18, 22))
    for s, v in enumerate((0.05, 0.9, 0.4, 0.7)):
        sites[s >> 1::2, s & 1::2] = v
    np.testing.assert_allclose(D.filter_x(sites, dn), sites, rtol=1e-13, atol=0)
    for work in ("f16", "f32"):
        D.assert_within_bound(O.cast_out(sites.astype(f32), work), D.filter_x(sites, dn), work, f"per-site {work}")


@pytest.mark.parametrize("radius", [1, 2])
def test_tiny_spatial_sigma_is_the_identity(rng, radius):
    """spatial_sigma = 0.05: every off-centre weight underflows, y = x; cast to the work dtype, the same bits."""
    x = rng.random((20, 30)).astype(f32)
    y = D.filter_x(x, RawDenoise(GAIN, READ, radius=radius, spatial_sigma=0.05))
    for work in ("f16", "f32"):
        assert np.array_equal(O.cast_out(x, work), y.astype(np.float16 if work == "f16" else np.float32))


@pytest.mark.parametrize("radius,factor", [(1, 0.6), (2, 0.55)])
def test_flat_patch_variance_drops(rng, radius, factor):
    """Poisson-Gaussian noise on a flat patch: the filtered variance is below `factor` of the input's (strength 1:
    0.54 at R = 1 and 0.49 at R = 2 measured on this seed's statistics)."""
    x = poisson_gaussian(rng, np.full((256, 256), 0.4))
    y = D.filter_x(x, RawDenoise(GAIN, READ, radius=radius))
    inner = np.s_[8:-8, 8:-8]
    assert y[inner].var() < factor * x[inner].var()


@pytest.mark.parametrize("radius", [1, 2])
def test_step_edge_is_preserved(rng, radius):
    """A 20-sigma step: pixels two or more sites (four raw pixels) from it move by less than one sigma against the
    filter of the same noise without the step."""
    sd = math.sqrt(GAIN * 0.3 + READ * READ)
    noise = rng.normal(0.0, sd, (64, 64))
    flat = 0.3 + noise
    step = flat.copy()
    step[:, 32:] += 20 * sd
    dn = RawDenoise(GAIN, READ, radius=radius)
    a, b = D.filter_x(flat, dn), D.filter_x(step, dn)
    assert np.abs(a[:, :28] - b[:, :28]).max() < sd
    assert np.abs(a[:, 36:] - (b[:, 36:] - 20 * sd)).max() < sd


@pytest.mark.parametrize("radius", [1, 2])
def test_listed_defect_does_not_reach_its_neighbours(rng, radius):
    x = poisson_gaussian(rng, np.full((24, 24), 0.3))
    mask = np.zeros((24, 24), bool)
    mask[11, 12] = mask[3, 3] = True
    dn = RawDenoise(GAIN, READ, radius=radius)
    hot, dead = x.copy(), x.copy()
    hot[mask], dead[mask] = 0.33, 0.27                   # (within the range kernel: a stuck 0 or 1 would barely show)
    a, b = D.filter_x(hot, dn, mask), D.filter_x(dead, dn, mask)
    assert np.array_equal(a[~mask], b[~mask])
    a, b = D.filter_x(hot, dn), D.filter_x(dead, dn)       # (without the map the value shows)
    assert not np.array_equal(a[~mask], b[~mask])


def test_step_one_mixes_sites():
    """The contract's taps are two pixels apart: taps one apart (the mutation the GPU tests catch) mix the sites."""
    x = np.empty((16, 16))
    for s, v in enumerate((0.1, 0.5, 0.5, 0.9)):
        x[s >> 1::2, s & 1::2] = v
    dn = RawDenoise(0.05, 0.3, strength=3.0)
    assert np.array_equal(D.filter_x(x, dn).astype(f32), x.astype(f32))
    assert not np.allclose(D.filter_x(x, dn, step=1), x, rtol=1e-3)


# ---- the noise model fit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("black", [None, 64, [60, 64, 70, 58]])
def test_noise_model_from_frames_recovers_the_model(rng, black):
    H, W, K = 256, 256, 8
    b = np.zeros((H, W)) if black is None else np.tile(np.reshape(black if np.ndim(black) else [black] * 4, (2, 2)),
                                                        (H // 2, W // 2))
    white = 4095
    xt = 0.02 + 0.88 * np.tile(np.linspace(0, 1, W), (H, 1))
    codes = [np.clip(np.rint(poisson_gaussian(rng, xt) * (white - b) + b), 0, 4095).astype(np.uint16) for _ in range(K)]
    gain, read = noise_model_from_frames(np.stack(codes), bits=12, black_level=black, white_level=white)
    assert abs(gain / GAIN - 1) < 0.1 and abs(read / READ - 1) < 0.1, (gain, read)


def test_noise_model_from_frames_rejects_bad_input():
    with pytest.raises(ValueError):
        noise_model_from_frames(np.zeros((1, 8, 8), np.uint16))
    with pytest.raises(ValueError):
        noise_model_from_frames(np.zeros((8, 8), np.uint16))
    with pytest.raises(ValueError):
        noise_model_from_frames(np.full((3, 8, 8), 100, np.uint16))           # one brightness level
    with pytest.raises(ValueError):
        noise_model_from_frames(np.zeros((3, 8, 8), np.uint16), black_level=5000)


# ---- settings ------------------------------------------------------------------------------------------------------------
def test_raw_denoise_settings():
    d = RawDenoise(0.01, 0.002)
    assert (d.strength, d.radius, d.spatial_sigma) == (1.0, 1, 1.0)
    assert RawDenoise(0, 1e-3, radius=2).gain == 0
    assert check_raw_denoise(None) is None and check_raw_denoise(d) is d
    for bad in ({"gain": -1e-3}, {"gain": math.inf}, {"gain": 1e39}, {"read_noise": 0.0}, {"read_noise": -1.0},
                {"read_noise": math.nan}, {"read_noise": 1e-50}, {"strength": 0.0}, {"strength": math.inf},
                {"spatial_sigma": 0.0}, {"spatial_sigma": -1.0}, {"radius": 0}, {"radius": 3}, {"radius": 1.0},
                {"radius": True}, {"gain": "1"}, {"gain": True}):
        kw = {"gain": 0.01, "read_noise": 0.002, **bad}
        with pytest.raises(ValueError):
            RawDenoise(**kw)
    for bad in (True, 1, (0.01, 0.002), "on"):
        with pytest.raises(ValueError):
            check_raw_denoise(bad)
    with pytest.raises(ValueError):
        camera_isp.Camera16(camera_isp.bayer.BayerPattern.RGGB, raw_denoise=(0.01, 0.002))


def test_denoise_entry_points_validate_on_the_host():
    """Every bad setting, shape, kind, dtype, level and pointer is refused before anything is launched (no device)."""
    from taichi_image_amd import _native
    L = _native.lib()
    good = _native.Denoise(0.01, 0.002, 1.0, 1.0, 1)
    fake = ctypes.c_void_p(0x1000)
    fake2 = ctypes.c_void_p(0x2000)

    def refused(rc):
        assert rc == 1                                           # (1: a host check; 2 would be a launch error)
        assert b"denoise" in L.mi_isp_last_error()

    for d in (_native.Denoise(0.01, 0.002, 1.0, 1.0, 0), _native.Denoise(0.01, 0.002, 1.0, 1.0, 3),
              _native.Denoise(-0.01, 0.002, 1.0, 1.0, 1), _native.Denoise(math.inf, 0.002, 1.0, 1.0, 1),
              _native.Denoise(0.01, 0.0, 1.0, 1.0, 1), _native.Denoise(0.01, math.nan, 1.0, 1.0, 1),
              _native.Denoise(0.01, 0.002, 0.0, 1.0, 1), _native.Denoise(0.01, 0.002, math.inf, 1.0, 1),
              _native.Denoise(0.01, 0.002, 1.0, -1.0, 1), _native.Denoise(0.01, 0.002, 1.0, math.nan, 1)):
        refused(L.mi_isp_denoise_cfa(fake, fake2, 8, 8, _native.MI_F16, d, None))
        refused(L.mi_isp_denoise_raw(fake, fake2, 8, 8, _native.MI_RAW_PACKED12, 0, _native.MI_F16, None, None, None, d,
                                     None))
    refused(L.mi_isp_denoise_cfa(fake, fake2, 8, 8, _native.MI_F16, None, None))
    refused(L.mi_isp_denoise_cfa(None, fake2, 8, 8, _native.MI_F16, good, None))
    refused(L.mi_isp_denoise_cfa(fake, fake, 8, 8, _native.MI_F16, good, None))           # in place
    refused(L.mi_isp_denoise_cfa(fake, fake2, -1, 8, _native.MI_F16, good, None))
    refused(L.mi_isp_denoise_cfa(fake, fake2, 8, 8, _native.MI_U8, good, None))
    raw = lambda *a: L.mi_isp_denoise_raw(*a)                                                # noqa: E731
    refused(raw(fake, fake2, 8, 8, 7, 0, _native.MI_F16, None, None, None, good, None))     # kind
    refused(raw(fake, fake2, 7, 8, _native.MI_RAW_PACKED12, 0, _native.MI_F16, None, None, None, good, None))   # odd
    refused(raw(fake, fake2, 8, 8, _native.MI_RAW_PACKED16, 1, _native.MI_F16, None, None, None, good, None))   # IDS
    refused(raw(fake, fake2, 8, 8, _native.MI_RAW_16U, 0, _native.MI_U16, None, None, None, good, None))        # dtype
    refused(raw(None, fake2, 8, 8, _native.MI_RAW_16U, 0, _native.MI_F16, None, None, None, good, None))
    refused(raw(fake, fake, 8, 8, _native.MI_RAW_16U, 0, _native.MI_F16, None, None, None, good, None))
    lv = _native.levels_arg([64] * 4, 4095)
    refused(raw(fake, fake2, 8, 8, _native.MI_RAW_32F, 0, _native.MI_F32, lv, None, None, good, None))  # levels, f32
    refused(raw(fake, fake2, 8, 8, _native.MI_RAW_PACKED12, 0, _native.MI_F16, _native.levels_arg([64] * 4, 5000),
                None, None, good, None))
    refused(raw(fake, fake2, 8, 8, _native.MI_RAW_PACKED12, 0, _native.MI_F16, None,
                _native.Shading(None, 4, 17, 13), None, good, None))                                   # no gains
    refused(raw(fake, fake2, 8, 8, _native.MI_RAW_PACKED12, 0, _native.MI_F16, None,
                _native.Shading(0x3000, 3, 17, 13), None, good, None))                                 # sites
    refused(raw(fake, fake2, 8, 8, _native.MI_RAW_PACKED12, 0, _native.MI_F16, None, None,
                _native.Defects(0x3000, 2, None), good, None))                                         # no mask
    ptrs = (ctypes.c_void_p * 2)(0x1000, None)
    outs = (ctypes.c_void_p * 2)(0x2000, 0x4000)
    refused(L.mi_isp_denoise_raw_batch(ptrs, outs, 2, 8, 8, _native.MI_RAW_PACKED12, 0, _native.MI_F16, None, None, None,
                                       good, None))
    assert L.mi_isp_version() >= 1700


def test_scan_cli_takes_the_settings():
    from taichi_image_amd.scripts import tonemap_scan
    a = tonemap_scan.build_parser().parse_args(["--images", "x", "--raw-denoise", "0.002", "0.006",
                                                "--denoise-strength", "1.5", "--denoise-radius", "2"])
    assert a.raw_denoise == [0.002, 0.006] and a.denoise_strength == 1.5 and a.denoise_radius == 2
    with pytest.raises(ValueError):                              # refused before any frame is read
        tonemap_scan.main(["--images", "/nonexistent", "--raw-denoise", "0.002", "0.006", "--denoise-radius", "3"])
