"""Dynamic defects without a GPU: the settings' validation (Python, full texts, and the C entry points' host-side checks on
made-up addresses), hand-derived vectors of the contract on its NumPy restatement (tests/dynamic_defects_ref.py), that the
frames the GPU tests use exercise the operator, and find_defects_dynamic's vote on hand-made flag planes."""
import ctypes

import numpy as np
import pytest
import torch

from taichi_image_amd import dynamic_defects as _stage  # noqa: F401  (the module under test: the file needs it as a whole)
from tests import dynamic_defects_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def dd():
    from taichi_image_amd import dynamic_defects
    return dynamic_defects


# ---- settings ----------------------------------------------------------------------------------------------------------
def test_settings_validation(dd):
    import taichi_image_amd as ti
    s = dd.DynamicDefects()
    assert (s.threshold, s.slope, s.tolerate, s.hot, s.dead) == (0.02, 0.2, 1, True, True)
    assert ti.DynamicDefects is dd.DynamicDefects and ti.find_defects_dynamic is dd.find_defects_dynamic
    assert dd.DynamicDefects(0.5, 0, 0, False, True).slope == 0
    with pytest.raises(Exception):
        s.threshold = 1.0                                                      # (frozen)
    for bad in (0, 0.0, -0.5, float("nan"), float("inf"), 1e39, 1e-50, "0.02", None, True):
        with pytest.raises(ValueError, match="DynamicDefects.threshold must be"):
            dd.DynamicDefects(threshold=bad)
    for bad in (-0.1, float("nan"), float("inf"), 1e39, "0.2", None, False):
        with pytest.raises(ValueError, match="DynamicDefects.slope must be"):
            dd.DynamicDefects(slope=bad)
    for bad in (2, -1, 0.0, 1.0, None, True, "1"):
        with pytest.raises(ValueError, match="DynamicDefects.tolerate must be 0 or 1"):
            dd.DynamicDefects(tolerate=bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="DynamicDefects.hot must be a bool"):
            dd.DynamicDefects(hot=bad)
        with pytest.raises(ValueError, match="DynamicDefects.dead must be a bool"):
            dd.DynamicDefects(dead=bad)
    assert dd.check_dynamic_defects(None) is None and dd.check_dynamic_defects(s) is s
    for bad in (True, 0.02, (0.02, 0.2), "on"):
        with pytest.raises(ValueError, match="dynamic_defects must be None or a DynamicDefects"):
            dd.check_dynamic_defects(bad)
    arg = dd.DynamicDefects(0.03, 0.25, 0, True, False)._arg()
    assert (f32(arg.threshold), f32(arg.slope), arg.tolerate, arg.hot, arg.dead) == (f32(0.03), f32(0.25), 0, 1, 0)


def test_the_full_error_texts(dd):
    cases = [
        (dict(threshold=-1), "DynamicDefects.threshold must be finite and > 0 (in f32 too), got -1"),
        (dict(threshold="a"), "DynamicDefects.threshold must be a number, got 'a'"),
        (dict(threshold=1e-50), "DynamicDefects.threshold must be finite and > 0 (in f32 too), got 1e-50"),
        (dict(slope=-0.5), "DynamicDefects.slope must be finite and >= 0 (in f32 too), got -0.5"),
        (dict(slope=1e39), "DynamicDefects.slope must be finite and >= 0 (in f32 too), got 1e+39"),
        (dict(tolerate=2), "DynamicDefects.tolerate must be 0 or 1, got 2"),
        (dict(hot=1), "DynamicDefects.hot must be a bool, got 1"),
        (dict(hot=False, dead=False), "DynamicDefects: at least one of hot and dead must be True"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError) as e:
            dd.DynamicDefects(**kw)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        dd.check_dynamic_defects("on")
    assert str(e.value) == "dynamic_defects must be None or a DynamicDefects, got str"
    x = np.zeros((4, 4), f32)
    with pytest.raises(ValueError, match="settings must be a DynamicDefects, got tuple"):
        dd.correct_cfa(x, (0.02, 0.2))
    with pytest.raises(ValueError, match="correct_cfa takes an f16 or f32 CFA, got"):
        dd.correct_cfa(np.zeros((4, 4), np.uint16))
    with pytest.raises(ValueError, match="defects must be None or a DefectMap, got list"):
        dd.correct_cfa(x, defects=[(0, 0)])
    from taichi_image_amd import DefectMap
    with pytest.raises(ValueError, match=r"the DefectMap is of a \(4, 6\) frame, the CFA is \(4, 4\)"):
        dd.correct_cfa(x, defects=DefectMap([(0, 0)], (4, 6)))
    stack = np.zeros((3, 4, 4), f32)
    for bad in (0, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="min_hits must be an integer in 1 .. 3"):
            dd.find_defects_dynamic(stack, dd.DynamicDefects(), bad)
    with pytest.raises(ValueError, match=r"frames must be \(K, H, W\), got shape \(4, 4\)"):
        dd.find_defects_dynamic(x, dd.DynamicDefects(), 1)
    with pytest.raises(ValueError, match="find_defects_dynamic takes f16 or f32 frames"):
        dd.find_defects_dynamic(np.zeros((3, 4, 4), np.uint16), dd.DynamicDefects(), 1)
    with pytest.raises(ValueError, match="settings must be a DynamicDefects, got float"):
        dd.find_defects_dynamic(stack, 0.02, 1)


# ---- the C entry points' host checks (made-up addresses: nothing is launched or dereferenced) ----------------------------
H, W = 4, 8
_bufs = [(ctypes.c_uint8 * 4096)() for _ in range(4)]
_addr = [ctypes.addressof(b) for b in _bufs]


def _ptrs(*addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


def _settings(threshold=0.02, slope=0.2, tolerate=1, hot=1, dead=1):
    from taichi_image_amd import _native
    return _native.DynamicDefects(threshold, slope, tolerate, hot, dead)


def _batch(L, settings=None, flags=None, lists=True, **over):
    from taichi_image_amd import _native
    a = dict(n=1, H=H, W=W, kind=_native.MI_RAW_16U, ids=0, work=_native.MI_F16, levels=None, shading=None, defects=None,
             plain=0, src=_addr[0], dst=_addr[1])
    a.update(over)
    s = _settings() if settings is None else settings
    return L.mi_isp_dynamic_defects_raw_batch(_ptrs(a["src"]) if lists else None, _ptrs(a["dst"]) if lists else None, a["n"],
                                              a["H"], a["W"], a["kind"], a["ids"], a["work"], a["levels"], a["shading"],
                                              a["defects"], ctypes.byref(s) if s is not False else None, a["plain"], None,
                                              flags)


def test_raw_batch_entry_rejects_on_the_host():
    from taichi_image_amd import _native
    L = _native.lib()
    grid = _native.Shading(_addr[3], 1, 2, 2)
    defect = _native.Defects(_addr[3], 3, None)                                # three listed pixels and no mask
    who = "dynamic_defects_raw_batch: "
    cases = [
        (dict(kind=5), "bad dynamic defects source kind 5"),
        (dict(kind=_native.MI_RAW_PACKED12, H=3), f"dynamic defects: packed frames must be even size, got 3x{W}"),
        (dict(kind=_native.MI_RAW_PACKED16, ids=1), "dynamic defects: the IDS layout is a packed-12 layout"),
        (dict(kind=_native.MI_RAW_32F, levels=_native.levels_arg([0] * 4, 100)),
         f"dynamic defects: levels apply to u16 codes only (source kind {_native.MI_RAW_32F})"),
        (dict(plain=1, shading=grid), "dynamic defects: the plain f32 output takes no shading grid"),
        (dict(defects=_ptrs(ctypes.addressof(defect))), "dynamic defects: frame 0: defects without a mask"),
        (dict(src=None), "dynamic defects: frame 0 has a null pointer"),
        (dict(dst=None), "dynamic defects: frame 0 has a null pointer"),
        (dict(dst=_addr[0]), "dynamic defects: frame 0: the CFA must not overwrite its source"),
        (dict(flags=_ptrs(_addr[1])), "dynamic defects: frame 0: the flags must not overwrite the source or the CFA"),
        (dict(lists=False), "dynamic defects: null frame list"),
        (dict(n=-1), "dynamic defects with -1 frames"),
        (dict(H=1 << 22), f"dynamic defects frame {1 << 22}x{W} too large"),
        (dict(H=-1), f"bad dynamic defects shape -1x{W}"),
        (dict(work=_native.MI_U8), "dynamic defects work dtype must be f16 or f32"),
        (dict(settings=False), "null dynamic defects settings"),
        (dict(settings=_settings(threshold=0.0)), "dynamic defects threshold 0 must be finite and > 0"),
        (dict(settings=_settings(threshold=float("nan"))), "dynamic defects threshold nan must be finite and > 0"),
        (dict(settings=_settings(slope=-1.0)), "dynamic defects slope -1 must be finite and >= 0"),
        (dict(settings=_settings(slope=float("inf"))), "dynamic defects slope inf must be finite and >= 0"),
        (dict(settings=_settings(tolerate=2)), "dynamic defects tolerate 2 (0 or 1)"),
        (dict(settings=_settings(hot=0, dead=0)), "dynamic defects with neither hot nor dead pixels to look for"),
    ]
    for bad, text in cases:
        assert _batch(L, **bad) == 1, bad
        assert L.mi_isp_last_error() == (who + text).encode(), bad
    assert _batch(L, n=0) == 0 and _batch(L, H=0) == 0 and _batch(L, n=0, lists=False) == 0      # nothing to do


def test_single_frame_entries_reject_on_the_host():
    from taichi_image_amd import _native
    L = _native.lib()
    s = _settings()
    raw = lambda src, dst, flags=None, st=s, **kw: L.mi_isp_dynamic_defects_raw(
        src, dst, kw.get("H", H), W, kw.get("kind", _native.MI_RAW_16U), 0, _native.MI_F32, None, None, None,
        ctypes.byref(st), 0, None, flags)
    assert raw(None, _addr[1]) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_raw: dynamic defects: frame 0 has a null pointer"
    assert raw(_addr[0], _addr[0]) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_raw: dynamic defects: frame 0: the CFA must not overwrite its source"
    assert raw(_addr[0], _addr[1], flags=_addr[0]) == 1
    assert L.mi_isp_last_error() == (b"dynamic_defects_raw: dynamic defects: frame 0: the flags must not overwrite the source "
                                     b"or the CFA")
    assert raw(_addr[0], _addr[1], kind=9) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_raw: bad dynamic defects source kind 9"
    assert raw(_addr[0], _addr[1], st=_settings(tolerate=-1)) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_raw: dynamic defects tolerate -1 (0 or 1)"
    assert raw(None, None, H=0) == 0
    cfa = lambda i, o, flags=None, st=s, dtype=_native.MI_F32, h=H: L.mi_isp_dynamic_defects_cfa(
        i, o, h, W, dtype, ctypes.byref(st) if st is not None else None, None, flags)
    assert cfa(None, _addr[1]) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_cfa: dynamic defects: null pointer"
    assert cfa(_addr[0], _addr[0]) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_cfa: dynamic defects: the output must not overwrite the input"
    assert cfa(_addr[0], _addr[1], flags=_addr[1]) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_cfa: dynamic defects: the flags must not overwrite the input or the output"
    assert cfa(_addr[0], _addr[1], dtype=_native.MI_U16) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_cfa: dynamic defects work dtype must be f16 or f32"
    assert cfa(_addr[0], _addr[1], st=None) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_cfa: null dynamic defects settings"
    assert cfa(_addr[0], _addr[1], st=_settings(threshold=-2.0)) == 1
    assert L.mi_isp_last_error() == b"dynamic_defects_cfa: dynamic defects threshold -2 must be finite and > 0"
    assert cfa(None, None, h=0) == 0


# ---- hand-derived vectors ----------------------------------------------------------------------------------------------
def frame6(taps, centre):
    """A 6 x 6 frame whose pixel (2, 2) has the value `centre` and the taps q0 .. q7 `taps`; every other pixel 0.25."""
    x = np.full((6, 6), 0.25, f32)
    for (dr, dc), v in zip(R.TAPS, taps):
        x[2 + dr, 2 + dc] = v
    x[2, 2] = centre
    return x


def taps_for(winner):
    """Taps whose pair `winner` (both 0.25) agrees best; the other three differ by 0.25, 0.375 and 0.3125 (all exact)."""
    q = [0.0] * 8
    others = [(0.125, 0.375), (0.125, 0.5), (0.0625, 0.375)]
    for i, (a, b) in enumerate(R.PAIRS):
        q[a], q[b] = (0.25, 0.25) if i == winner else others.pop()
    return q


@pytest.mark.parametrize("winner", [0, 1, 2, 3])
@pytest.mark.parametrize("tolerate", [0, 1])
def test_each_direction_wins_once(winner, tolerate):
    """The hot centre 1.0 over taps of at most 0.5: x - hi >= 0.5 > T(hi) <= 0.02 + 0.2 * 0.5; y is the winning pair's mean
    0.25, below hi (0.5 or 0.375, the largest and the second largest tap)."""
    d = R.detect(frame6(taps_for(winner), 1.0), tolerate=tolerate)
    assert d.n[2, 2] == 8 and d.hot[2, 2] and not d.dead[2, 2]
    assert d.hi[2, 2] == f32(0.5 if tolerate == 0 else 0.375)
    assert d.pair[2, 2] == winner and d.y[2, 2] == f32(0.25) and not d.clamped[2, 2]
    # the same taps under a dead centre: lo is 0.0625 (0.125 with tolerate), the centre -1 is far below, y = 0.25 again
    d = R.detect(frame6(taps_for(winner), -1.0), tolerate=tolerate)
    assert d.dead[2, 2] and not d.hot[2, 2] and d.lo[2, 2] == f32(0.0625 if tolerate == 0 else 0.125)
    assert d.pair[2, 2] == winner and d.y[2, 2] == f32(0.25)
    # hot only / dead only
    assert not R.detect(frame6(taps_for(winner), 1.0), tolerate=tolerate, hot=False).flags[2, 2]
    assert not R.detect(frame6(taps_for(winner), -1.0), tolerate=tolerate, dead=False).flags[2, 2]


def test_a_tie_goes_to_the_earlier_pair():
    # (q1, q6) = (0.25, 0.375) and (q3, q4) = (0.5, 0.375) both differ by 0.125; the diagonals differ by more
    q = [0.0] * 8
    q[1], q[6], q[3], q[4], q[0], q[7], q[2], q[5] = 0.25, 0.375, 0.5, 0.375, 0.125, 0.5, 0.0625, 0.375
    d = R.detect(frame6(q, 2.0), tolerate=0)
    assert d.hot[2, 2] and d.pair[2, 2] == 0 and d.y[2, 2] == f32(0.3125)
    q[3], q[4], q[1], q[6] = 0.25, 0.375, 0.5, 0.375                           # the other way round: still the earlier
    d = R.detect(frame6(q, 2.0), tolerate=0)
    assert d.pair[2, 2] == 0 and d.y[2, 2] == f32(0.4375)


def test_the_threshold_is_strict_and_grows_with_the_signal():
    # every tap 0.5: T = f32(f32(0.25) + f32(f32(0.5) * f32(0.5))) = 0.5 exactly; x - hi = 0.5 is not hot, one ulp more is
    x = frame6([0.5] * 8, 1.0)
    assert not R.detect(x, threshold=0.25, slope=0.5).flags.any()
    x[2, 2] = np.nextafter(f32(1.0), f32(2.0))
    d = R.detect(x, threshold=0.25, slope=0.5)
    assert d.hot[2, 2] and d.y[2, 2] == f32(0.5)
    # a negative neighbourhood: max(v, 0) = 0, T = t; the taps -1, the centre -0.5: x - hi = 0.5 > 0.25
    d = R.detect(frame6([-1.0] * 8, -0.5), threshold=0.25, slope=0.5)
    assert d.hot[2, 2] and d.y[2, 2] == f32(-1.0)


def test_the_clamp_with_a_hot_partner_in_the_chosen_pair():
    """Pixel (0, 2) of a 4 x 6 frame keeps q3 q4 q5 q6 q7 (0.25, 1.0, 0.25, 0.3125, 0.25) and one usable pair, (q3, q4) = (0.25, 1.0): its partner (0, 4) is
    hot too.  tolerate=1: hi is the second largest tap 0.3125, m = 0.625 > hi, y = hi."""
    x = np.full((4, 6), 0.25, f32)
    x[0, 2], x[0, 4] = 1.0, 1.0
    x[2, 2] = 0.3125
    d = R.detect(x, tolerate=1)
    assert d.n[0, 2] == 5 and d.hot[0, 2] and d.pair[0, 2] == 1 and d.m[0, 2] == f32(0.625)
    assert d.hi[0, 2] == f32(0.3125) and d.y[0, 2] == f32(0.3125) and d.clamped[0, 2]
    assert d.hot[0, 4] and d.y[0, 4] == f32(0.3125)                            # (its taps: q3 q5 q6 = 1.0, 0.3125, 0.25; no usable pair)
    d0 = R.detect(x, tolerate=0)                                               # tolerate=0 sees the partner as the scene
    assert not d0.flags.any() and np.array_equal(d0.y, x)


def test_too_few_taps_leave_the_pixel_alone():
    x = np.full((2, 4), 0.25, f32)
    x[0, 0] = 1.0                                                              # its one tap is (0, 2), and the other way round
    d = R.detect(x, tolerate=1)                                                # n = 1 < 3
    assert d.n.max() == 1 and not d.flags.any() and np.array_equal(d.y, x)
    # tolerate=0, n = 1 >= 1: (0, 0) is hot (0.75 > T(0.25) = 0.07), no usable pair, y = hi; (0, 2) is dead against it
    # (0.75 > T(1.0) = 0.22), y = lo: both tests read the input frame x, not each other's y
    d = R.detect(x, tolerate=0)
    assert d.hot[0, 0] and d.pair[0, 0] == -1 and d.y[0, 0] == f32(0.25)
    assert d.dead[0, 2] and d.pair[0, 2] == -1 and d.y[0, 2] == f32(1.0) and d.flags.sum() == 2
    assert not R.detect(x, tolerate=0, dead=False).flags[0, 2] and not R.detect(x, tolerate=0, hot=False).flags[0, 0]
    one = np.full((1, 1), 5.0, f32)
    assert np.array_equal(R.detect(one, tolerate=0).y, one)                    # n = 0


def test_non_finite_taps_are_dropped_and_non_finite_centres_kept():
    q = taps_for(1)                                                            # (q3, q4) agrees best
    q[0], q[7], q[1] = np.nan, np.inf, -np.inf                                 # the vertical and one diagonal pair go
    d = R.detect(frame6(q, 1.0), tolerate=1)
    assert d.n[2, 2] == 5 and d.hot[2, 2] and d.pair[2, 2] == 1 and d.y[2, 2] == f32(0.25)
    q = taps_for(0)
    q[3] = np.nan                                                              # (q3, q4) is gone, the vertical pair stays
    assert R.detect(frame6(q, 1.0)).pair[2, 2] == 0
    for v in (np.nan, np.inf, -np.inf):
        d = R.detect(frame6(taps_for(0), v))
        assert not d.flags[2, 2] and np.array_equal(d.y[2, 2], f32(v), equal_nan=True)


def test_a_listed_centre_is_kept_and_a_listed_tap_is_not_one():
    x = frame6(taps_for(0), 1.0)
    listed = np.zeros((6, 6), bool)
    listed[2, 2] = True
    d = R.detect(x, excluded=listed)
    assert not d.flags[2, 2] and d.y[2, 2] == f32(1.0)
    assert d.n[2, 4] == 4 and d.listed_tap[2, 4] and not d.listed_tap[2, 2]    # (2, 4): q1 q6 of 3 columns, minus the centre
    listed[:] = False
    listed[0, 2] = True                # q1: the vertical pair goes; the next best is (q2, q5) = (0.125, 0.375), m = 0.25
    d = R.detect(x, excluded=listed)
    assert d.n[2, 2] == 7 and d.hot[2, 2] and d.pair[2, 2] == 3 and d.y[2, 2] == f32(0.25)


def test_mask_words_layout():
    from taichi_image_amd import DefectMap
    m = DefectMap([(0, 0), (1, 31), (2, 32), (3, 69), (65, 33)], (66, 70))
    assert np.array_equal(R.mask_words(m.mask()), m.mask_words())
    assert R.mask_words(np.ones((3, 33), bool)).tolist() == [[0xFFFFFFFF, 1]] * 3


# ---- the inputs exercise the operator ----------------------------------------------------------------------------------
FRAMES = [(66, 70), (67, 69), (64, 64), (66, 96)]            # the shapes of tests/test_gpu_dynamic_defects.py of 4096 pixels or more


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("top", [4095, 65535, 1000])
def test_the_frames_exercise_the_operator(rng, H, W, top):
    """Three frames in a row from the tests' generator (a GPU test draws up to three from one rng), in the code ranges of
    every source kind: all the injections are found with tolerate=1, the pairs are missed with tolerate=0, each of the
    operator's arms runs, and the scene without injections has no flagged pixel."""
    clean_rng = np.random.default_rng(20260)
    for k in range(3):
        codes, info = R.make_frame(rng, H, W, top)
        x = codes.astype(f32) * f32(1.0 / top)
        listed = R.listed_mask(info, H, W)
        for excluded in (None, listed):
            R.assert_exercised(x, f"{H}x{W} top {top} frame {k}", excluded=excluded)
            d1 = R.detect(x, excluded=excluded)
            d0 = R.detect(x, tolerate=0, excluded=excluded)
            injected = np.zeros((H, W), bool)
            for a, b in info.hot + info.dead + info.pairs:
                injected[a, b] = True
            assert np.array_equal(d1.flags, injected), "tolerate=1 finds the injections and nothing else"
            assert all(d1.hot[a, b] for a, b in info.hot + info.pairs) and all(d1.dead[a, b] for a, b in info.dead)
            missed = [p for p in info.pairs if not d0.flags[p]]
            assert len(missed) >= 1 and not (d0.flags & ~injected).any()
        # the thin line stays: no pixel of its column changes but the injected ones
        assert np.array_equal(d1.y[:, R.LINE_COL][~injected[:, R.LINE_COL]], x[:, R.LINE_COL][~injected[:, R.LINE_COL]])
        line = x[H // 2 - 8:H // 2 + 8, R.LINE_COL].astype(np.float64) - x[H // 2 - 8:H // 2 + 8, R.LINE_COL - 2]
        assert line.mean() > 0.12, "the line is bright enough to be flagged if it were one pixel"
        clean, _ = R.make_frame(clean_rng, H, W, top, inject=False)
        xc = clean.astype(f32) * f32(1.0 / top)
        for tolerate in (0, 1):
            for excluded in (None, listed):
                d = R.detect(xc, tolerate=tolerate, excluded=excluded)
                assert not d.flags.any() and np.array_equal(d.y, xc), "the scene alone must flag nothing"


def test_small_frames_take_what_fits(rng):
    for H, W in [(2, 4), (6, 4), (1, 5)]:
        codes, info = R.make_frame(rng, H, W)
        assert codes.shape == (H, W) and all(a < H and b < W for a, b in info.hot + info.dead + info.pairs + info.listed)


# ---- the vote ----------------------------------------------------------------------------------------------------------
def test_the_vote_on_hand_made_flag_planes(dd):
    H, W, K = 4, 70, 5
    hits = np.zeros((K, H, W), bool)
    hits[:, 0, 0] = True                                                       # 5 of 5
    hits[:4, 1, 31] = True                                                     # 4 of 5: bit 31, the sign bit of an i32 word
    hits[1:4, 2, 32] = True                                                    # 3 of 5
    hits[4, 3, 69] = True                                                      # 1 of 5: the last column, in the third word
    hits[::2, 3, 64] = True                                                    # 3 of 5
    words = torch.from_numpy(np.stack([R.mask_words(h) for h in hits]).view(np.int32))
    assert words.shape == (K, H, 3)
    assert np.array_equal(dd._unpack_flags(words, W).numpy().astype(bool), hits)
    for min_hits in range(1, K + 1):
        got = dd._vote(words, W, min_hits).numpy()
        assert got.shape == (H, W) and np.array_equal(got, hits.sum(axis=0) >= min_hits), min_hits
    assert sorted(map(tuple, np.argwhere(dd._vote(words, W, 4).numpy()))) == [(0, 0), (1, 31)]
