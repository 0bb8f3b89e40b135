"""Green equalisation without a GPU: the settings' validation, the host checks of the three C entry points with their full
error texts (made-up addresses: nothing is launched), and the reference of tests/green_equalize_ref.py against a scalar
restatement of the contract, hand-derived vectors, what it must leave alone and what it achieves."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import isp_oracle as O
from taichi_image_amd import _native
from taichi_image_amd._native import MI_F16, MI_RAW_16U, MI_RAW_32F, MI_RAW_PACKED12, MI_RAW_PACKED16
from tests import green_equalize_ref as R

f32 = np.float32
PATTERNS = [O.RGGB, O.GRBG, O.GBRG, O.BGGR]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ge():
    from taichi_image_amd import green_equalize
    return green_equalize


def header_constants():
    """TILE_H, TILE_W and MAX_FRAMES of csrc/isp_green_equalize.h."""
    text = open(os.path.join(ROOT, "taichi_image_amd", "csrc", "isp_green_equalize.h")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) for name in ("TILE_H", "TILE_W", "MAX_FRAMES"))


TILE_H, TILE_W, MAX_FRAMES = 64, 64, 32
SHAPES = [(2, 2), (3, 5), (6, 6), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (TILE_H + 7, 2 * TILE_W + 3)]


def test_the_shapes_are_the_headers():
    assert header_constants() == (TILE_H, TILE_W, MAX_FRAMES)
    from tests import test_gpu_green_equalize as G
    assert (G.TILE_H, G.TILE_W, G.MAX_FRAMES) == (TILE_H, TILE_W, MAX_FRAMES) and G.SHAPES == SHAPES


# ---- the settings ------------------------------------------------------------------------------------------------------
def test_settings_validation(ge):
    s = ge.GreenEqualize()
    assert (s.threshold, s.slope, s.strength, s.radius, s.edge) == (1 / 256, 1 / 16, 1.0, 1, 4.0)
    ge.GreenEqualize(threshold=0, slope=0, strength=0, radius=2, edge=0)       # every lower bound is allowed
    ge.GreenEqualize(strength=1, radius=np.int64(2), threshold=np.float32(0.5))
    for name in ("threshold", "slope", "edge"):
        for bad in (-1e-9, float("nan"), float("inf"), 1e39, True, "1", None):
            with pytest.raises(ValueError, match=f"GreenEqualize.{name}"):
                ge.GreenEqualize(**{name: bad})
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="GreenEqualize.strength"):
            ge.GreenEqualize(strength=bad)
    for bad in (0, 3, 1.0, True, "1", None):
        with pytest.raises(ValueError, match="GreenEqualize.radius"):
            ge.GreenEqualize(radius=bad)
    with pytest.raises(Exception):
        s.radius = 2                                                           # frozen
    assert ge.check_green_equalize(None) is None and ge.check_green_equalize(s) is s
    for bad in (True, False, 1, "on", dict()):
        with pytest.raises(ValueError, match="green_equalize must be None or a GreenEqualize"):
            ge.check_green_equalize(bad)
    a = ge.GreenEqualize(0.01, 0.02, 0.5, 2, 3.0)._arg()
    assert (a.threshold, a.slope, a.strength, a.radius, a.edge) == (f32(0.01), f32(0.02), 0.5, 2, 3.0)
    with pytest.raises(ValueError, match="settings must be a GreenEqualize"):
        ge.equalize_cfa(np.zeros((2, 2), f32), __import__("taichi_image_amd").BayerPattern.RGGB, settings=1)
    with pytest.raises(ValueError, match="pattern must be a BayerPattern"):
        ge.equalize_cfa(np.zeros((2, 2), f32), 0)
    with pytest.raises(ValueError, match="f16 or f32"):
        ge.equalize_cfa(np.zeros((2, 2), np.uint16), __import__("taichi_image_amd").BayerPattern.RGGB)


def test_the_camera_option_is_validated():
    import taichi_image_amd as ti
    for cam in (ti.Camera16, ti.Camera32):
        with pytest.raises(ValueError, match="green_equalize must be None or a GreenEqualize"):
            cam(ti.BayerPattern.RGGB, green_equalize=True)


# ---- the C entry points' host checks -----------------------------------------------------------------------------------
H0, W0 = 4, 8
_bufs = [(ctypes.c_uint8 * 4096)() for _ in range(4)]        # disjoint planes, each larger than any 4 x 8 frame
_addr = [ctypes.addressof(b) for b in _bufs]


def _ptrs(*addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


GOOD = dict(n=1, H=H0, W=W0, kind=MI_RAW_16U, ids=0, work=MI_F16, pattern=0, levels=None, shading=None, defects=None,
            plain=0, src=_addr[0], dst=_addr[1], s=(1 / 256, 1 / 16, 1.0, 1, 4.0))
_grid = _native.Shading(_addr[2], 1, 2, 2)
_defect = _native.Defects(_addr[2], 3, None)                 # three listed pixels and no mask


def _batch(L, a):
    s = _native.GreenEqualize(*a["s"]) if a["s"] is not None else None
    d = None if a["defects"] is None else _ptrs(ctypes.addressof(a["defects"]))
    return L.mi_isp_green_equalize_raw_batch(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], a["kind"], a["ids"],
                                             a["work"], a["pattern"], a["levels"], a["shading"], d, s, a["plain"], None)


def _single(L, a):
    s = _native.GreenEqualize(*a["s"]) if a["s"] is not None else None
    return L.mi_isp_green_equalize_raw(a["src"], a["dst"], a["H"], a["W"], a["kind"], a["ids"], a["work"], a["pattern"],
                                       a["levels"], a["shading"], a["defects"], s, a["plain"], None)


def _cfa(L, a):
    s = _native.GreenEqualize(*a["s"]) if a["s"] is not None else None
    return L.mi_isp_green_equalize_cfa(a["src"], a["dst"], a["H"], a["W"], a["work"], a["pattern"], s, None)


def _setting(**kw):
    base = dict(threshold=1 / 256, slope=1 / 16, strength=1.0, radius=1, edge=4.0)
    base.update(kw)
    return dict(s=tuple(base.values()))


SETTINGS_CASES = [
    (dict(s=None), "null green equalize settings"),
    (_setting(threshold=-1.0), "green equalize threshold -1 must be finite and >= 0"),
    (_setting(threshold=float("nan")), "green equalize threshold nan must be finite and >= 0"),
    (_setting(slope=float("inf")), "green equalize slope inf must be finite and >= 0"),
    (_setting(slope=-0.5), "green equalize slope -0.5 must be finite and >= 0"),
    (_setting(strength=1.5), "green equalize strength 1.5 must be in [0, 1]"),
    (_setting(strength=-0.5), "green equalize strength -0.5 must be in [0, 1]"),
    (_setting(strength=float("nan")), "green equalize strength nan must be in [0, 1]"),
    (_setting(radius=0), "green equalize radius 0 (1 or 2)"),
    (_setting(radius=3), "green equalize radius 3 (1 or 2)"),
    (_setting(edge=-2.0), "green equalize edge -2 must be finite and >= 0"),
    (_setting(edge=float("inf")), "green equalize edge inf must be finite and >= 0"),
    (dict(pattern=4), "bad green equalize pattern 4"),
    (dict(pattern=-1), "bad green equalize pattern -1"),
    (dict(H=-1), f"bad green equalize shape -1x{W0}"),
    (dict(H=1 << 22), f"green equalize frame {1 << 22}x{W0} too large"),
    (dict(work=1), "green equalize work dtype must be f16 or f32"),
]
RAW_CASES = [
    (dict(kind=5), "bad green equalize source kind 5"),
    (dict(kind=MI_RAW_PACKED12, H=3), f"green equalize: packed frames must be even size, got 3x{W0}"),
    (dict(kind=MI_RAW_PACKED16, ids=1), "green equalize: the IDS layout is a packed-12 layout"),
    (dict(kind=MI_RAW_32F, levels=_native.levels_arg([0] * 4, 100)),
     f"green equalize: levels apply to u16 codes only (source kind {MI_RAW_32F})"),
    (dict(plain=1, shading=_grid), "green equalize: the plain f32 output takes no shading grid"),
    (dict(defects=_defect), "green equalize: frame 0: defects without a mask"),
    (dict(src=None), "green equalize: frame 0 has a null pointer"),
    (dict(dst=_addr[0]), "green equalize: frame 0: the CFA must not overwrite its source"),
]


@pytest.mark.parametrize("entry,who", [(_batch, "green_equalize_raw_batch"), (_single, "green_equalize_raw"),
                                       (_cfa, "green_equalize_cfa")])
def test_the_full_error_texts(entry, who):
    L = _native.lib()
    cases = list(SETTINGS_CASES)
    if entry is _cfa:
        cases += [(dict(src=None), "green equalize: null pointer"),
                  (dict(dst=_addr[0]), "green equalize: the output must not overwrite the input")]
    else:
        cases += RAW_CASES
    for bad, text in cases:
        assert entry(L, {**GOOD, **bad}) == 1, (who, text)
        assert L.mi_isp_last_error() == f"{who}: {text}".encode(), (who, text)
    assert _batch(L, {**GOOD, "n": -1}) == 1
    assert L.mi_isp_last_error() == b"green_equalize_raw_batch: green equalize with -1 frames"


def test_nothing_to_do_succeeds_without_a_launch():
    L = _native.lib()
    assert _batch(L, {**GOOD, "n": 0}) == 0
    for entry in (_batch, _single, _cfa):
        assert entry(L, {**GOOD, "H": 0}) == 0 and entry(L, {**GOOD, "W": 0}) == 0
        assert entry(L, {**GOOD, "H": 0, "src": None, "dst": None}) == 0


# ---- the reference against a scalar restatement of the contract -------------------------------------------------------
def scalar(x, pattern, threshold, slope, strength, radius, edge, listed=None):
    """The contract pixel by pixel, in np.float32 scalars."""
    H, W = x.shape
    gp = 1 if pattern in (O.RGGB, O.BGGR) else 0
    if radius == 1:
        offs_o = [(-1, -1), (-1, 1), (1, -1), (1, 1)]
        offs_s = [(0, 0), (-2, 0), (0, -2), (0, 2), (2, 0)]
    else:
        offs_o = [(dy, dx) for dy in (-3, -1, 1, 3) for dx in (-3, -1, 1, 3)]
        offs_s = [(0, 0)] + [(dy, dx) for dy in (-2, 0, 2) for dx in (-2, 0, 2) if (dy, dx) != (0, 0)]
    t, s, e_f, hs = f32(threshold), f32(slope), f32(edge), f32(strength) * f32(0.5)
    y = x.copy()

    def kept(r, c):
        return 0 <= r < H and 0 <= c < W and not (listed is not None and listed[r, c]) and np.isfinite(x[r, c])

    def group(r, c, offs):
        vals = [x[r + dy, c + dx] for dy, dx in offs if kept(r + dy, c + dx)]
        total = None
        for v in vals:
            total = v if total is None else f32(total + v)
        return total, len(vals), (max(vals) if vals else None), (min(vals) if vals else None)

    with np.errstate(all="ignore"):
        for r in range(H):
            for c in range(W):
                if ((r + c) & 1) != gp or not kept(r, c):
                    continue
                so, no, xo, io = group(r, c, offs_o)
                ss, ns, xs_, is_ = group(r, c, offs_s)
                if no < 1:
                    continue
                mo, ms = f32(so / f32(no)), f32(ss / f32(ns))
                d = f32(mo - ms)
                lim = f32(t + f32(s * max(mo, ms)))
                e = f32(e_f * lim)
                if abs(d) <= lim and f32(xo - io) <= e and f32(xs_ - is_) <= e:
                    y[r, c] = f32(x[r, c] + f32(hs * d))
    return y


def wide_range_frame(rng, H, W):
    """Values whose sums depend on their order (magnitudes over 2^8) and whose gates go both ways."""
    return (rng.uniform(0.2, 0.3, (H, W)) * np.exp2(rng.integers(-4, 5, (H, W)) * (rng.random((H, W)) < 0.15))).astype(f32)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_reference_is_the_contract_pixel_by_pixel(rng, pattern, radius):
    applied = 0
    for H, W in [(2, 2), (3, 5), (6, 6), (11, 14)]:
        for k in range(3):
            x = wide_range_frame(rng, H, W) if k else R.flat_field(rng, H, W, pattern)
            listed = None
            if k == 2:
                listed = rng.random((H, W)) < 0.1
                x[rng.random((H, W)) < 0.05] = np.nan
                x[rng.random((H, W)) < 0.03] = np.inf
                x[rng.random((H, W)) < 0.03] = -np.inf
            kw = dict(threshold=0.01, slope=0.25, strength=0.7, radius=radius, edge=6.0)
            q = R.equalize(x, pattern, excluded=listed, **kw)
            want = scalar(x, pattern, listed=listed, **kw)
            assert np.array_equal(q.y.view(np.uint32), want.view(np.uint32)), (H, W, k)
            applied += int(q.apply.sum())
    assert applied > 50


def test_the_sum_order_matters_on_these_frames(rng):
    """The frames of the test above tell a sum in another order apart: reversing group S's taps changes bits."""
    x = wide_range_frame(rng, 11, 14)
    odd, even = R.taps(2)
    a = R._group(np.pad(x, 3, constant_values=-np.inf), 11, 14, even)[0]
    b = R._group(np.pad(x, 3, constant_values=-np.inf), 11, 14, even[::-1])[0]
    assert not np.array_equal(a, b)
    assert R.taps(1) == ([(-1, -1), (-1, 1), (1, -1), (1, 1)], [(0, 0), (-2, 0), (0, -2), (0, 2), (2, 0)])
    assert len(odd) == 16 and len(even) == 9 and odd[:5] == [(-3, -3), (-3, -1), (-3, 1), (-3, 3), (-1, -3)]
    assert even[:5] == [(0, 0), (-2, -2), (-2, 0), (-2, 2), (0, -2)]


# ---- hand-derived vectors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_flat_imbalanced_field_comes_out_balanced(pattern, radius):
    g, eps = 0.25, 0.02
    x = R.flat_field(None, 16, 18, pattern, g, eps, sigma=0.0)
    q = R.equalize(x, pattern, radius=radius)
    sign = R.phase_sign(pattern, 16, 18)
    inner = np.zeros_like(q.green)
    inner[3:-3, 3:-3] = True                                                   # (at the frame's edge the groups lose taps)
    assert q.apply[q.green].all()
    hi, lo = q.y[(sign > 0) & inner], q.y[(sign < 0) & inner]
    assert np.abs(hi - f32(g)).max() <= 1e-6 * g and np.abs(lo - f32(g)).max() <= 1e-6 * g
    assert np.array_equal(q.y[~q.green].view(np.uint32), x[~q.green].view(np.uint32))
    half = R.equalize(x, pattern, radius=radius, strength=0.5).y                # half the strength: half the way
    assert np.abs(half[(sign > 0) & inner] - f32(g * (1 + eps / 2))).max() <= 1e-6 * g
    assert np.array_equal(R.equalize(x, pattern, radius=radius, strength=0.0).y, x)


@pytest.mark.parametrize("radius", [1, 2])
def test_all_four_patterns_agree_on_shifted_frames(rng, radius):
    """The frame under GRBG is the RGGB frame shifted by one column: the results are each other's shifts; RGGB and BGGR
    (and GRBG and GBRG) share their green sites and give the same result on the same frame."""
    big = R.make_scene(rng, 40, 47, O.RGGB).astype(f32)
    a = R.equalize(big[:, :-1], O.RGGB, radius=radius)
    b = R.equalize(big[:, :-1], O.BGGR, radius=radius)
    assert np.array_equal(a.y, b.y) and a.apply.any()
    inner = (slice(None), slice(4, -4))                                        # (away from the columns the shift cuts)
    c = R.equalize(big[:, 1:], O.GRBG, radius=radius)
    d = R.equalize(big[:, 1:], O.GBRG, radius=radius)
    assert np.array_equal(c.y, d.y)
    assert np.array_equal(a.y[:, 1:][inner], c.y[:, :-1][inner])
    assert R.green_parity(O.RGGB) == 1 == R.green_parity(O.BGGR) and R.green_parity(O.GRBG) == 0 == R.green_parity(O.GBRG)


def _two_level(H, W, pattern, a, b):
    """Greens of even rows a, of odd rows b, the other sites 0.125."""
    sign = R.phase_sign(pattern, H, W)
    return np.where(sign > 0, a, np.where(sign < 0, b, 0.125)).astype(f32)


@pytest.mark.parametrize("radius", [1, 2])
def test_the_gates_hold_at_equality(radius):
    """|d| == lim applies, the next f32 below for lim does not; a range of exactly e applies, one ulp less of e does not."""
    x = _two_level(12, 12, O.RGGB, 0.5, 0.25)                                  # every sum is exact: |d| = 0.25
    mid = (slice(4, 8), slice(4, 8))
    on = R.equalize(x, O.RGGB, threshold=0.25, slope=0.0, radius=radius)
    assert on.apply[mid][on.green[mid]].all() and (on.y[mid][on.green[mid]] == f32(0.375)).all()
    below = np.nextafter(f32(0.25), f32(0))
    off = R.equalize(x, O.RGGB, threshold=below, slope=0.0, radius=radius)
    assert not off.apply.any() and np.array_equal(off.y, x)
    # the range gates: the own phase of the pixel at (5, 6) spans exactly 0.25 (one tap raised), |d| stays below lim
    x = _two_level(12, 12, O.RGGB, 0.5, 0.5)
    x[5, 8] = 0.75
    assert R.green_parity(O.RGGB) == (5 + 6) & 1
    on = R.equalize(x, O.RGGB, threshold=0.25, slope=0.0, edge=1.0, radius=radius)
    assert on.apply[5, 6] and on.ok_s[5, 6]
    off = R.equalize(x, O.RGGB, threshold=0.25, slope=0.0, edge=np.nextafter(f32(1), f32(0)), radius=radius)
    assert not off.apply[5, 6] and not off.ok_s[5, 6] and off.ok_d[5, 6] and off.ok_o[5, 6]
    assert off.y[5, 6] == x[5, 6]
    # ... and the other phase's: (4, 7) has (5, 8) in group O and not in group S
    assert on.apply[4, 7] and on.ok_o[4, 7]
    assert not off.apply[4, 7] and not off.ok_o[4, 7] and off.ok_d[4, 7] and off.ok_s[4, 7]


def test_the_correction_rounds_in_three_steps(rng):
    """y = x + (f32(strength) 0.5f) d: the halved strength, the product and the add round once each.  On a noisy field
    the fused form (one rounding for product and add) gives other bits somewhere, so the frames tell them apart."""
    x = R.flat_field(rng, 32, 32, O.RGGB)
    q = R.equalize(x, O.RGGB, strength=0.3)
    hs = f32(f32(0.3) * f32(0.5))
    want = (x + (hs * q.d).astype(f32)).astype(f32)
    assert q.apply.sum() > 400 and np.array_equal(q.y[q.apply], want[q.apply])
    fused = (x.astype(np.float64) + np.float64(hs) * q.d.astype(np.float64)).astype(f32)
    assert (fused[q.apply] != want[q.apply]).any()


# ---- what the reference does not touch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_step_edge_and_a_texture_keep_their_bits(rng, pattern, radius):
    H, W = 24, 26
    reach = 2 if radius == 1 else 3
    x = np.where(np.arange(W)[None, :] < 13, 0.1, 0.5).astype(f32) * np.ones((H, 1), f32)
    q = R.equalize(x, pattern, radius=radius)
    straddle = slice(13 - reach, 13 + reach)                                   # the windows that reach across the step
    assert np.array_equal(q.y[:, straddle].view(np.uint32), x[:, straddle].view(np.uint32))
    assert not q.apply[:, straddle].any()
    x = np.where(rng.random((H, W)) < 0.5, 0.3, 0.5).astype(f32)
    q = R.equalize(x, pattern, radius=radius)
    flat = (q.n_o > 0) & (np.abs(q.d) <= q.lim) & q.ok_o & q.ok_s              # (a window that happens to hold one level)
    assert np.array_equal(q.y[~flat].view(np.uint32), x[~flat].view(np.uint32)) and flat.mean() < 0.05
    assert np.array_equal(q.y, x)                                              # (one level throughout: d = 0)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_frames_smaller_than_the_window(rng, pattern, radius):
    for H, W in [(2, 2), (3, 5), (6, 6), (1, 1), (1, 7)]:
        x = R.flat_field(rng, H, W, pattern, sigma=0.001)
        q = R.equalize(x, pattern, radius=radius)
        assert q.y.shape == (H, W) and np.isfinite(q.y).all()
        assert np.array_equal(q.y[~q.green], x[~q.green])
        if H >= 2 and W >= 2:
            assert q.apply[q.green].all(), (H, W)                              # every green site has a kept tap in O
            sign = R.phase_sign(pattern, H, W)
            assert abs(q.y[sign > 0].mean() - q.y[sign < 0].mean()) < 0.25 * abs(x[sign > 0].mean() - x[sign < 0].mean())
        else:
            assert not q.apply.any() and np.array_equal(q.y, x)               # (no other phase in reach: nO = 0)


def test_listed_and_non_finite_pixels(rng):
    x = R.flat_field(rng, 12, 12, O.GRBG, sigma=0.001)
    listed = np.zeros((12, 12), bool)
    listed[4, 4] = listed[5, 7] = True
    x[6, 6], x[7, 3], x[2, 8] = np.nan, np.inf, -np.inf
    q = R.equalize(x, O.GRBG, excluded=listed)
    for p in [(4, 4), (5, 7), (6, 6), (7, 3), (2, 8)]:
        assert q.green[p] and not q.apply[p]
        assert q.y[p].view(np.uint32) == x[p].view(np.uint32)
    assert q.n_s[4, 6] == 3 and q.n_o[5, 5] == 2 and q.n_o[6, 8] == 3        # neighbours lose them as taps ...
    assert q.apply[4, 6] and q.apply[5, 5] and np.isfinite(q.y[q.apply]).all()   # ... and are corrected from the rest
    free = R.equalize(x, O.GRBG)
    assert free.n_s[4, 6] == 4 and not np.array_equal(free.y, q.y)


# ---- what it achieves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("eps", [0.01, 0.02])
def test_the_imbalance_goes_and_the_noise_does_not_grow(radius, eps):
    """256 x 256 at g = 0.25, Gr and Gb at +-eps, Gaussian noise of sigma = 0.005, default settings, seeds 0 .. 7."""
    for seed in range(8):
        x = R.flat_field(np.random.default_rng(seed), 256, 256, O.RGGB, 0.25, eps, 0.005)
        q = R.equalize(x, O.RGGB, radius=radius)
        sign = R.phase_sign(O.RGGB, 256, 256)
        gr, gb = sign > 0, sign < 0
        before = abs(float(x[gr].mean(dtype=np.float64)) - float(x[gb].mean(dtype=np.float64)))
        after = abs(float(q.y[gr].mean(dtype=np.float64)) - float(q.y[gb].mean(dtype=np.float64)))
        assert after <= 0.02 * before, (seed, after / before)
        assert q.apply[q.green].mean() >= 0.99, (seed, q.apply[q.green].mean())
        assert q.y[gr].var(dtype=np.float64) <= x[gr].var(dtype=np.float64), seed


# ---- no vacuous inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_generated_frames_exercise_the_operator(rng, pattern, radius):
    for H, W in SHAPES:
        for top in (4095, 65535, 1000):
            x = R.make_frame(rng, H, W, pattern, top).astype(f32) * f32(1 / top)
            R.assert_exercised(x, pattern, f"{H}x{W} top={top}", radius=radius)
    x = R.make_frame(rng, TILE_H + 7, 2 * TILE_W + 3, pattern).astype(f32) * f32(1 / 4095)
    q = R.equalize(x, pattern, radius=radius)
    cov = R.coverage(q)
    assert cov["apply"] >= 0.25 and min(cov["only_d"], cov["only_o"], cov["only_s"]) >= 0.01, cov
    assert not np.array_equal(q.y, x)
    ends = [int(round(f * x.shape[1])) for f in R.BANDS]
    assert np.array_equal(q.y[:, ends[2] + 3:], x[:, ends[2] + 3:]) or q.apply[:, ends[2] + 3:].mean() < 0.02
