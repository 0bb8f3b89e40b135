"""Temporal noise reduction without a GPU: the settings' and the C entry points' checks, the history= rules, and the
contract's properties on its NumPy restatement (tests/temporal_ref.py): a hand-computed vector, the two exact properties,
the noise reduction on a static scene and a moving edge without a ghost."""
import ctypes
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from tests import temporal_ref as T

f32 = np.float32
GAIN, READ_NOISE = 2.4e-4, 1.5e-3


@pytest.fixture(scope="module")
def tn():
    from taichi_image_amd import temporal
    return temporal


# ---- settings and arguments ----------------------------------------------------------------------------------------------
def test_settings_validation(tn):
    s = tn.TemporalDenoise(GAIN, READ_NOISE)
    assert (s.threshold, s.max_weight) == (3.0, 0.75)
    tn.TemporalDenoise(0, 1e-3, threshold=0.5, max_weight=0)                   # gain 0 and max_weight 0 are allowed
    tn.TemporalDenoise(np.float32(0.1), np.float64(0.1), 2, np.float32(0.5))   # NumPy scalars and ints are numbers
    bad = [dict(gain=-1e-9), dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=1e39), dict(gain=True),
           dict(gain="1"), dict(gain=None),
           dict(read_noise=0), dict(read_noise=-1.0), dict(read_noise=float("nan")), dict(read_noise=1e39),
           dict(read_noise=1e-30),                                             # (its square is 0 in f32)
           dict(read_noise=1e30),                                              # (its square is inf in f32)
           dict(read_noise=False), dict(read_noise=[1.0]),
           dict(threshold=0), dict(threshold=-3.0), dict(threshold=float("inf")), dict(threshold=True),
           dict(threshold=1e-30), dict(threshold="3"),
           dict(max_weight=1.0), dict(max_weight=-0.1), dict(max_weight=float("nan")), dict(max_weight=1 - 1e-12),
           dict(max_weight=True), dict(max_weight=None)]
    for kw in bad:
        args = dict(gain=GAIN, read_noise=READ_NOISE)
        args.update(kw)
        with pytest.raises(ValueError, match="TemporalDenoise"):
            tn.TemporalDenoise(**args)
    assert tn.check_temporal_denoise(None) is None and tn.check_temporal_denoise(s) is s
    for v in (True, 0.5, "on", (GAIN, READ_NOISE)):
        with pytest.raises(ValueError, match="temporal_denoise"):
            tn.check_temporal_denoise(v)


def test_package_exports():
    import taichi_image_amd as ti
    for name in ("TemporalDenoise", "TemporalHistory", "check_temporal_denoise", "temporal_cfa"):
        assert getattr(ti, name) is getattr(ti.temporal, name)


def test_c_entry_points_reject_bad_arguments_before_any_launch():
    from taichi_image_amd import _native
    L = _native.lib()
    bufs = [(ctypes.c_float * 16)() for _ in range(4)]
    pa, ph, po, pc = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)           # (made up: never dereferenced)

    def settings(gain=GAIN, read_noise=READ_NOISE, threshold=3.0, max_weight=0.75):
        return _native.Temporal(gain, read_noise, threshold, max_weight)

    def rejected(rc):
        assert rc != 0
        assert b"temporal" in L.mi_isp_last_error(), L.mi_isp_last_error()

    F32 = _native.MI_F32
    cfa = lambda **kw: L.mi_isp_temporal_cfa(  # noqa: E731
        kw.get("src", pa), kw.get("hin", ph), kw.get("hout", po), kw.get("dst", pc), kw.get("H", 4), kw.get("W", 4),
        kw.get("dtype", F32), kw.get("s", settings()), None)
    rejected(cfa(s=None))
    for kw in (dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(read_noise=0.0),
               dict(read_noise=-1.0), dict(read_noise=float("nan")), dict(read_noise=1e-30), dict(read_noise=1e30),
               dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("inf")), dict(threshold=1e-30),
               dict(max_weight=1.0), dict(max_weight=-0.5), dict(max_weight=float("nan")), dict(max_weight=2.0)):
        rejected(cfa(s=settings(**kw)))
    rejected(cfa(dtype=_native.MI_U16))
    rejected(cfa(src=None))
    rejected(cfa(dst=None))
    rejected(cfa(hout=None))
    rejected(cfa(dst=pa))                                                      # in place
    rejected(cfa(hout=ph))                                                     # the new history over the old one
    rejected(cfa(hout=pa))                                                     # ... over the source
    rejected(cfa(hout=pc))                                                     # ... over the output
    rejected(cfa(hout=ctypes.c_void_p(ph.value + 8), H=2, W=2))                # a partial overlap
    rejected(cfa(H=-1))
    raw = lambda **kw: L.mi_isp_temporal_raw(  # noqa: E731
        kw.get("src", pa), kw.get("hin", ph), kw.get("hout", po), kw.get("dst", pc), kw.get("H", 4), kw.get("W", 4),
        kw.get("kind", _native.MI_RAW_32F), kw.get("ids", 0), kw.get("work", F32), kw.get("levels"), kw.get("shading"),
        None, kw.get("s", settings()), kw.get("plain", 0), None)
    rejected(raw(s=settings(max_weight=1.0)))
    rejected(raw(s=None))
    rejected(raw(kind=7))
    rejected(raw(work=_native.MI_U8))
    rejected(raw(src=None))
    rejected(raw(hout=None))
    rejected(raw(dst=None))                                                    # (a NULL CFA takes out_f32_plain)
    rejected(raw(dst=pa))
    rejected(raw(hout=ph))
    rejected(raw(hout=pa))
    rejected(raw(hout=pc))
    rejected(raw(kind=_native.MI_RAW_PACKED12, H=3))                           # packed: even sizes
    rejected(raw(ids=1))                                                       # IDS is a packed-12 layout
    rejected(raw(levels=_native.levels_arg([0, 0, 0, 0], 4095)))               # levels: u16 codes only
    rejected(raw(shading=_native.Shading(pa, 1, 2, 2), plain=1))               # plain y takes no grid
    srcs, hins, houts, outs = ((ctypes.c_void_p * 2)(p, ctypes.c_void_p(p.value + 32)) for p in (pa, ph, po, pc))
    batch = lambda n, H, W, s=None, houts=houts, hins=hins: L.mi_isp_temporal_raw_batch(  # noqa: E731
        srcs, hins, houts, outs, n, H, W, _native.MI_RAW_32F, 0, F32, None, None, None, s or settings(), 0, None)
    rejected(batch(-1, 2, 2))
    rejected(batch(0, 2, 2, settings(threshold=0.0)))                          # (checked even for no frames)
    rejected(batch(2, 2, 2, houts=(ctypes.c_void_p * 2)(po, po)))              # two frames, one new plane
    rejected(batch(2, 2, 2, houts=(ctypes.c_void_p * 2)(po, ph)))              # frame 1 writes frame 0's history
    rejected(batch(2, 2, 2, houts=(ctypes.c_void_p * 2)(po, None)))
    # n == 0 and H * W == 0 are successful no-ops
    assert batch(0, 2, 2) == 0 and batch(2, 0, 4) == 0 and batch(2, 4, 0) == 0
    assert cfa(H=0) == 0 and raw(W=0) == 0


def test_history_object(tn):
    h = tn.TemporalHistory()
    assert h.frames == 0 and h.shape is None and h.device is None and h.plane is None
    with pytest.raises(AttributeError):
        h.frames = 3
    h.reset()
    assert h.frames == 0


def _used_history(tn, shape):
    """A history that has seen frames of `shape` on cuda:0, made without a device."""
    h = tn.TemporalHistory()
    h._shape, h._device = shape, torch.device("cuda", 0)
    return h


@pytest.mark.parametrize("cam", ["Camera16", "Camera32"])
def test_history_rules_are_checked_before_anything_is_uploaded(tn, cam):
    """Every rejection happens on host tensors: nothing has touched a device."""
    import taichi_image_amd as ti
    with pytest.raises(ValueError, match="temporal_denoise"):
        getattr(ti, cam)(ti.BayerPattern.RGGB, temporal_denoise=True)
    on = getattr(ti, cam)(ti.BayerPattern.RGGB, temporal_denoise=ti.TemporalDenoise(GAIN, READ_NOISE))
    off = getattr(ti, cam)(ti.BayerPattern.RGGB)
    assert on.temporal_denoise == ti.TemporalDenoise(GAIN, READ_NOISE) and off.temporal_denoise is None
    p12 = torch.zeros((4, 6), dtype=torch.uint8)
    p16 = torch.zeros((4, 8), dtype=torch.uint8)
    u16 = torch.zeros((4, 4), dtype=torch.uint16)
    f = torch.zeros((4, 4), dtype=torch.float32)
    a, b = ti.TemporalHistory(), ti.TemporalHistory()
    # on, and no history
    for call in (lambda: on.load_packed12(p12), lambda: on.load_packed16(p16), lambda: on.load_16u(u16),
                 lambda: on.load_16f(u16), lambda: on.load_32f(f), lambda: on.load_packed12_batch([p12, p12]),
                 lambda: on.load_packed16_batch([p16]), lambda: on.load_packed12_batch([p12, p12], history=[a]),
                 lambda: on.load_packed12_batch([p12, p12], history=[a, None]),
                 lambda: on.process_packed12([p12]), lambda: on.load_packed12_batch([], history=[a])):
        with pytest.raises(ValueError, match="history="):
            call()
    with pytest.raises(ValueError, match="TemporalHistory"):
        on.load_packed12(p12, history="camera 0")
    with pytest.raises(ValueError, match="list"):
        on.load_packed12_batch([p12], history=a)
    # off, and a history
    for call in (lambda: off.load_packed12(p12, history=a), lambda: off.load_packed16(p16, history=a),
                 lambda: off.load_16u(u16, history=a), lambda: off.load_16f(u16, history=a),
                 lambda: off.load_32f(f, history=a), lambda: off.load_packed12_batch([p12], history=[a]),
                 lambda: off.load_packed16_batch([p16], history=[a]), lambda: off.load_packed12_batch([], history=[]),
                 lambda: off.process_packed12([p12], history=[a])):
        with pytest.raises(ValueError, match="temporal_denoise is off"):
            call()
    # one object twice
    with pytest.raises(ValueError, match="twice"):
        on.load_packed12_batch([p12, p12], history=[a, a])
    with pytest.raises(ValueError, match="twice"):
        on.process_packed12([p12, p12, p12], history=[a, b, a])
    # another shape, another device
    other = _used_history(tn, (6, 4))
    for call in (lambda: on.load_packed12(p12, history=other), lambda: on.load_32f(f, history=other),
                 lambda: on.load_packed16_batch([p16, p16], history=[a, other])):
        with pytest.raises(ValueError, match=r"reset\(\)"):
            call()
    moved = _used_history(tn, (4, 4))
    moved._device = torch.device("cuda", 1)
    with pytest.raises(ValueError, match=r"reset\(\)"):
        on.load_16u(u16, history=moved)
    for h in (a, b, other, moved):
        assert h.frames == 0 and h.plane is None
    # set(): None leaves it, False turns it off, a TemporalDenoise replaces it
    on.set(temporal_denoise=None)
    assert on.temporal_denoise is not None
    on.set(temporal_denoise=ti.TemporalDenoise(0.0, 0.01, max_weight=0.5))
    assert on.temporal_denoise.max_weight == 0.5
    with pytest.raises(ValueError, match="temporal_denoise"):
        on.set(temporal_denoise=True)
    on.set(temporal_denoise=False)
    assert on.temporal_denoise is None
    with pytest.raises(ValueError, match="temporal_denoise is off"):
        on.load_packed12(p12, history=a)
    # temporal_cfa's own arguments
    with pytest.raises(ValueError, match="TemporalDenoise"):
        tn.temporal_cfa(np.zeros((4, 4), f32), a, (GAIN, READ_NOISE))
    with pytest.raises(ValueError, match="TemporalHistory"):
        tn.temporal_cfa(np.zeros((4, 4), f32), None, ti.TemporalDenoise(GAIN, READ_NOISE))
    with pytest.raises(ValueError, match="f16 or f32"):
        tn.temporal_cfa(np.zeros((4, 4), np.uint16), a, ti.TemporalDenoise(GAIN, READ_NOISE))
    with pytest.raises(ValueError, match=r"reset\(\)"):
        tn.temporal_cfa(np.zeros((4, 4), f32), other, ti.TemporalDenoise(GAIN, READ_NOISE))


# ---- the contract on the reference ---------------------------------------------------------------------------------------
def test_hand_computed_vector():
    """A 6 x 4 frame, h = 1/2 everywhere, gain 0, read_noise 1/4 (var = 1/16), threshold 2 (c = 4, c var = 1/4),
    max_weight 1/2; x = h + e / 64.  Every value below is a dyadic rational that f32 holds, so each f32 operation is
    exact - except m = D R[6], rounded by hand.  (3, 3) and (5, 1) are listed defects."""
    e = np.zeros((6, 4))
    e[0::2, 0::2] = [[2, 1], [0.5, 0.5], [1, 1]]            # the even-even site plane: rows 0, 2, 4 x columns 0, 2
    e[1::2, 1::2] = [[1, -3], [2, 100], [100, 2]]           # the odd-odd one: rows 1, 3, 5 x columns 1, 3
    h = np.full((6, 4), 0.5, f32)
    x = (h + (e / 64).astype(f32)).astype(f32)
    listed = np.zeros((6, 4), bool)
    listed[3, 3] = listed[5, 1] = True
    s = T.Settings(0.0, 0.25, threshold=2.0, max_weight=0.5)
    w, n = T.weights(x, h, s, listed)
    y = T.blend(x, h, s, listed)

    def by_hand(D, rcp, xe):
        m = D * rcp                                          # D R[n]
        qv = (m * m) / (4 * Fr(1, 16))                       # (m m) / (c var)
        wt = Fr(1, 2) * max(1 - qv, 0)
        xv = Fr(1, 2) + Fr(xe) / 64
        return wt, (xv if wt == 0 else xv + wt * (Fr(1, 2) - xv))

    # the corner (0, 0): taps (0, 0) (0, 2) (2, 0) (2, 2), n = 4, D = (2 + 1 + 1/2 + 1/2) / 64 = 1/16, m = 1/64
    wt, yv = by_hand(Fr(4, 64), Fr(1, 4), 2)
    assert n[0, 0] == 4 and w[0, 0] == float(wt) == 1023 / 2048 and y[0, 0] == float(yv)
    assert yv == Fr(1, 2) + Fr(2, 64) * Fr(1025, 2048)
    # the edge (2, 0): rows 0, 2, 4 x columns 0, 2, n = 6, D = 6/64; R[6] = 11184811 / 2^26, D R[6] = (2^26 + 2) / 2^32,
    # which rounds to the 24-bit 2^26 / 2^32 = 1/64
    assert float(s.R[6]) == 11184811 / 2 ** 26
    wt, yv = by_hand(Fr(6, 64), Fr(1, 6), 0.5)               # (m = 1/64 after the rounding: the exact 1/6 gives it)
    assert n[2, 0] == 6 and w[2, 0] == float(wt) == 1023 / 2048 and y[2, 0] == float(yv)
    # (3, 1): rows 1, 3, 5 x columns 1, 3 without the listed (3, 3) and (5, 1): n = 4, D = (1 + 3 + 2 + 2) / 64 = 1/8
    wt, yv = by_hand(Fr(8, 64), Fr(1, 4), 2)
    assert n[3, 1] == 4 and w[3, 1] == float(wt) == 255 / 512 and y[3, 1] == float(yv) == 0.5 + 257 / 16384
    assert n[1, 1] == 3                                      # (rows 1, 3 x columns 1, 3 without (3, 3))
    # with the two taps counted the pixel would have been dropped: they never feed a neighbour's metric
    assert T.weights(x, h, s)[0][3, 1] == 0 and T.blend(x, h, s)[3, 1] == x[3, 1]
    # the listed centre (3, 3) is filtered like any other pixel, on the same four taps, from its own value
    wt, yv = by_hand(Fr(8, 64), Fr(1, 4), 100)
    assert n[3, 3] == 4 and w[3, 3] == float(wt) and y[3, 3] == float(yv) == 10521 / 8192
    # every other site plane has x == h: D = 0, w = max_weight, y = x
    assert np.all(w[0::2, 1::2] == 0.5) and np.array_equal(y[0::2, 1::2], x[0::2, 1::2])


def test_a_pixel_without_taps_keeps_x():
    x = np.array([[0.25, 0.5], [0.75, 1.0]], f32)
    h = np.array([[0.26, 0.5], [0.7, 0.0]], f32)
    listed = np.array([[True, False], [False, False]])
    s = T.Settings(GAIN, 0.1)
    w, n = T.weights(x, h, s, listed)
    assert n.tolist() == [[0, 1], [1, 1]]
    y = T.blend(x, h, s, listed)
    assert y[0, 0] == x[0, 0] and y[0, 1] == x[0, 1] and y[1, 1] == x[1, 1] and y[1, 0] != x[1, 0]


def test_exact_property_no_past(rng):
    """max_weight = 0 and an empty history both give y = x bit for bit."""
    x = T.noisy(rng, T.smooth_scene(34, 38), GAIN, READ_NOISE)
    h = T.noisy(rng, T.smooth_scene(34, 38), GAIN, READ_NOISE)
    x[3, 5] = -0.0                                                             # (the sign of a zero survives too)
    y = T.blend(x, h, T.Settings(GAIN, READ_NOISE, max_weight=0.0))
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
    y = T.blend(x, None, T.Settings(GAIN, READ_NOISE))
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
    assert not np.array_equal(T.blend(x, h, T.Settings(GAIN, READ_NOISE)), x)  # (the settings do filter this pair)


def test_exact_property_motion_leaves_no_ghost(rng):
    """A pixel whose kept taps all differ from the history by more than threshold * sqrt(var) has w = 0 and y = x."""
    H, W = 40, 44
    s = T.Settings(GAIN, READ_NOISE)
    h = T.noisy(rng, T.smooth_scene(H, W), GAIN, READ_NOISE)
    sd = np.sqrt(float(s.gain) * np.maximum(h.astype(np.float64), 0) + float(s.rn2))
    sign = np.where(rng.random((H, W)) < 0.5, -1.0, 1.0)
    x = (h + sign * (3.0 * sd.max() * 1.02 + rng.random((H, W)) * 0.1)).astype(f32)
    moved = np.abs(x.astype(np.float64) - h) > 3.0 * sd.max()                  # (more than the threshold at every tap)
    assert moved.all()
    w, _ = T.weights(x, h, s)
    assert np.all(w == 0)
    assert np.array_equal(T.blend(x, h, s).view(np.uint32), x.view(np.uint32))


def test_noise_reduction_on_a_static_scene():
    """A smooth 128 x 128 scene with noise from the model, the default settings: after 40 frames the residual noise power
    over 10 more frames is 0.202 of the input's (DESIGN.md 3 records it; a weight of exactly max_weight would give
    (1 - 0.75) / (1 + 0.75) = 0.143)."""
    rng = np.random.default_rng(1234)
    clean = T.smooth_scene(128, 128).astype(f32)
    s = T.Settings(GAIN, READ_NOISE)
    h, ratios = None, []
    for k in range(50):
        x = T.noisy(rng, clean, GAIN, READ_NOISE)
        h = T.blend(x, h, s)
        if k >= 40:
            ratios.append(np.mean((h.astype(np.float64) - clean) ** 2) / np.mean((x.astype(np.float64) - clean) ** 2))
    ratio = float(np.mean(ratios))
    print(f"static scene: residual noise power ratio {ratio:.4f}")
    assert ratio < 0.25
    assert ratio > 0.143                                                       # (no better than the linear filter)


def test_a_moving_step_edge_leaves_no_ghost():
    """Codes 0.1 | 0.7, the edge moved 16 columns between two frames: every pixel at least 2 columns inside the strip that
    changed side is returned untouched, and the rest of the frame keeps averaging."""
    rng = np.random.default_rng(4321)
    H, W, c0, c1 = 64, 96, 40, 56
    s = T.Settings(GAIN, READ_NOISE)
    first = np.full((H, W), 0.1)
    first[:, c0:] = 0.7
    second = np.full((H, W), 0.1)
    second[:, c1:] = 0.7
    x0, x1 = T.noisy(rng, first, GAIN, READ_NOISE), T.noisy(rng, second, GAIN, READ_NOISE)
    h = T.blend(x0, None, s)
    w, _ = T.weights(x1, h, s)
    y = T.blend(x1, h, s)
    strip = slice(c0 + 2, c1 - 2)
    assert np.array_equal(y[:, strip].view(np.uint32), x1[:, strip].view(np.uint32)) and np.all(w[:, strip] == 0)
    outside = np.concatenate([w[:, :c0], w[:, c1:]], axis=1)
    print(f"moving edge: mean weight outside the strip {outside.mean():.4f}")
    assert outside.mean() > 0.75 / 2


@pytest.mark.parametrize("H,W", [(64, 64), (66, 70), (130, 66)])
def test_the_generated_frames_exercise_the_operator(rng, H, W):
    """The frames the GPU tests use put at least 10 % of a frame of 4096 pixels or more in each weight class, and every
    pixel with w > 0 and h != x changes."""
    frames = [f.astype(f32) for f in T.make_sequence(rng, H, W, 3, GAIN, READ_NOISE)]
    s = T.Settings(GAIN, READ_NOISE)
    ys = T.run(frames, s)
    for k in (1, 2):
        none, some, most, changes = T.coverage(frames[k], ys[k - 1], s)
        print(f"{H}x{W} frame {k}: w == 0 {none:.3f}, partial {some:.3f}, above half {most:.3f}")
        assert min(none, some, most) >= 0.10 and changes
    # the third output depends on the first frame, through the history
    other = T.run([frames[0] + f32(0.004), frames[1], frames[2]], s)
    assert not np.array_equal(other[2], ys[2])


def test_the_rounding_frame_tells_the_tap_orders_apart(rng):
    """The frame the GPU tests use for the order of the sum: on the reference, the reversed order changes more than 5 % of
    its pixels (the noise-model frames do not tell the orders apart at all)."""
    x, h, s = T.rounding_frame(rng, 66, 70)
    w, _ = T.weights(x, h, s)
    assert ((w > 0) & (w < f32(0.75))).mean() > 0.5
    y, other = T.blend(x, h, s), T.blend(x, h, s, taps=T.TAPS[::-1])
    assert (y != other).mean() > 0.05
