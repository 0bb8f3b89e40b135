"""Exposure merge ("Exposure merge") without a GPU: the settings, the C entries' and the loaders' checks
(all made before anything is uploaded or launched), and the contract on the NumPy reference tests/exposure_merge_ref.py - a
hand-computed vector, the exact properties, the noise on a static scene, a moved block, and that the generated brackets
exercise the operator."""
import ctypes
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from tests import exposure_merge_ref as M

f32 = np.float32
GAIN, READ_NOISE = 2.4e-4, 1.5e-3
RATIOS = {2: (1, 4), 3: (1, 4, 16), 4: (1, 2, 4, 8)}          # the ratios of the kernel tests, by E
BRACKET_LOADERS = ("load_packed12_bracket", "load_packed16_bracket", "load_16u_bracket", "load_16f_bracket",
                   "load_32f_bracket", "load_packed12_bracket_batch", "load_packed16_bracket_batch")


@pytest.fixture(scope="module")
def em():
    from taichi_image_amd import exposure_merge
    return exposure_merge


# ---- settings and arguments ----------------------------------------------------------------------------------------------
def test_settings_validation(em):
    s = em.ExposureMerge((1, 4, 16), GAIN, READ_NOISE)
    assert (s.ratios, s.saturation, s.knee, s.threshold, s.exposures) == ((1.0, 4.0, 16.0), 0.9, 0.25, 4.0, 3)
    em.ExposureMerge([1, 2], 0, 1e-3, saturation=4000.0, knee=1, threshold=0.5)    # gain 0 and knee 1 are allowed; a list
    em.ExposureMerge(np.array([1.0, 1.5, 2.0, 65536.0]), np.float32(0.1), np.float64(0.1), 1, np.float32(0.5), 2)
    bad = [dict(ratios=(1,)), dict(ratios=(1, 2, 3, 4, 5)), dict(ratios=()), dict(ratios=4), dict(ratios="14"),
           dict(ratios=None), dict(ratios=(2, 4)), dict(ratios=(1, 1)), dict(ratios=(1, 4, 4)), dict(ratios=(1, 4, 2)),
           dict(ratios=(1, float("nan"))), dict(ratios=(1, float("inf"))), dict(ratios=(1, 65537)), dict(ratios=(1, True)),
           dict(ratios=(1, "4")), dict(ratios=(1, 1 + 1e-12)),                   # (equal in f32)
           dict(ratios=np.ones((2, 2))),
           dict(gain=-1e-9), dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=1e39), dict(gain=True),
           dict(gain="1"), dict(gain=None),
           dict(read_noise=0), dict(read_noise=-1.0), dict(read_noise=float("nan")), dict(read_noise=1e39),
           dict(read_noise=1e-30),                                             # (its square is 0 in f32)
           dict(read_noise=1e30),                                              # (its square is inf in f32)
           dict(read_noise=False), dict(read_noise=[1.0]),
           dict(saturation=0), dict(saturation=-0.9), dict(saturation=float("inf")), dict(saturation=True),
           dict(saturation=1e-46),                                             # (0 in f32)
           dict(saturation=1e-39, knee=1e-3),                                  # (1 / (saturation * knee) is inf in f32)
           dict(knee=0), dict(knee=-0.25), dict(knee=1.0001), dict(knee=float("nan")), dict(knee=True), dict(knee="1"),
           dict(threshold=0), dict(threshold=-3.0), dict(threshold=float("inf")), dict(threshold=True),
           dict(threshold=1e-30), dict(threshold="3")]
    for kw in bad:
        args = dict(ratios=(1, 4), gain=GAIN, read_noise=READ_NOISE)
        args.update(kw)
        with pytest.raises(ValueError, match="ExposureMerge"):
            em.ExposureMerge(**args)
    assert em.check_exposure_merge(None) is None and em.check_exposure_merge(s) is s
    for v in (True, 0.5, "on", ((1, 4), GAIN, READ_NOISE)):
        with pytest.raises(ValueError, match="exposure_merge"):
            em.check_exposure_merge(v)
    a = s._arg()
    assert a.n == 3 and list(a.ratio) == [1.0, 4.0, 16.0, 0.0] and a.saturation == f32(0.9) and a.knee == 0.25


def test_package_exports():
    import taichi_image_amd as ti
    for name in ("ExposureMerge", "check_exposure_merge", "merge_cfa"):
        assert getattr(ti, name) is getattr(ti.exposure_merge, name)
    for cam in (ti.Camera16, ti.Camera32):
        for name in BRACKET_LOADERS + ("exposure_merge",):
            assert hasattr(cam, name)


def test_c_entry_points_reject_bad_arguments_before_any_launch():
    from taichi_image_amd import _native
    L = _native.lib()
    bufs = [(ctypes.c_float * 64)() for _ in range(4)]
    pa, pb, pc, po = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)           # (made up: never dereferenced)

    def settings(ratios=(1, 4), gain=GAIN, read_noise=READ_NOISE, saturation=0.9, knee=0.25, threshold=4.0, n=None):
        r = list(ratios) + [0.0] * (4 - len(ratios))
        return _native.ExposureMerge(len(ratios) if n is None else n, (ctypes.c_float * 4)(*r), gain, read_noise,
                                     saturation, knee, threshold)

    def rejected(rc):
        assert rc != 0
        assert b"exposure merge" in L.mi_isp_last_error(), L.mi_isp_last_error()

    F32 = _native.MI_F32
    two = (ctypes.c_void_p * 2)(pa, pb)
    cfa = lambda **kw: L.mi_isp_merge_cfa(  # noqa: E731
        kw.get("src", two), kw.get("dst", po), kw.get("H", 4), kw.get("W", 4), kw.get("dtype", F32),
        kw.get("s", settings()), None)
    rejected(cfa(s=None))
    for kw in (dict(n=1), dict(n=5), dict(n=0), dict(ratios=(2, 4)), dict(ratios=(1, 1)), dict(ratios=(1, 4, 2)),
               dict(ratios=(1, float("nan"))), dict(ratios=(1, float("inf"))), dict(ratios=(1, 65537.0)),
               dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(read_noise=0.0),
               dict(read_noise=-1.0), dict(read_noise=float("nan")), dict(read_noise=1e-30), dict(read_noise=1e30),
               dict(saturation=0.0), dict(saturation=-1.0), dict(saturation=float("inf")),
               dict(saturation=1e-39, knee=1e-3), dict(knee=0.0), dict(knee=1.5), dict(knee=float("nan")),
               dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("inf")), dict(threshold=1e-30)):
        rejected(cfa(s=settings(**kw)))
    rejected(cfa(dtype=_native.MI_U16))
    rejected(cfa(src=None))
    rejected(cfa(dst=None))
    rejected(cfa(src=(ctypes.c_void_p * 2)(pa, None)))
    rejected(cfa(dst=pa))                                                      # over frame 0
    rejected(cfa(dst=pb))                                                      # over frame 1
    rejected(cfa(dst=ctypes.c_void_p(pb.value + 8), H=2, W=2))                 # a partial overlap
    rejected(cfa(H=-1))
    three = (ctypes.c_void_p * 3)(pa, pb, None)                                # three ratios, and frame 2 is NULL
    rejected(cfa(src=three, s=settings((1, 4, 16))))
    raw = lambda **kw: L.mi_isp_merge_raw(  # noqa: E731
        kw.get("src", two), kw.get("dst", po), kw.get("H", 4), kw.get("W", 4), kw.get("kind", _native.MI_RAW_32F),
        kw.get("ids", 0), kw.get("work", F32), kw.get("levels"), kw.get("shading"), None, kw.get("s", settings()),
        kw.get("plain", 0), None)
    rejected(raw(s=settings(knee=2.0)))
    rejected(raw(s=None))
    rejected(raw(kind=7))
    rejected(raw(work=_native.MI_U8))
    rejected(raw(src=None))
    rejected(raw(dst=None))
    rejected(raw(dst=pb))
    rejected(raw(kind=_native.MI_RAW_PACKED12, H=3))                           # packed: even sizes
    rejected(raw(ids=1))                                                       # IDS is a packed-12 layout
    rejected(raw(levels=_native.levels_arg([0, 0, 0, 0], 4095)))               # levels: u16 codes only
    rejected(raw(shading=_native.Shading(pa, 1, 2, 2), plain=1))               # plain y takes no grid
    srcs = (ctypes.c_void_p * 4)(pa, pb, ctypes.c_void_p(pa.value + 64), ctypes.c_void_p(pb.value + 64))
    outs = (ctypes.c_void_p * 2)(po, ctypes.c_void_p(po.value + 64))
    batch = lambda n, H, W, s=None, outs=outs, srcs=srcs: L.mi_isp_merge_raw_batch(  # noqa: E731
        srcs, outs, n, H, W, _native.MI_RAW_32F, 0, F32, None, None, None, s or settings(), 0, None)
    rejected(batch(-1, 2, 2))
    rejected(batch(0, 2, 2, settings(threshold=0.0)))                          # (checked even for no brackets)
    rejected(batch(2, 2, 2, outs=(ctypes.c_void_p * 2)(po, po)))               # two brackets, one output
    rejected(batch(2, 2, 2, outs=(ctypes.c_void_p * 2)(po, pa)))               # bracket 1 writes bracket 0's frame
    rejected(batch(2, 2, 2, outs=(ctypes.c_void_p * 2)(po, None)))
    rejected(batch(2, 2, 2, srcs=(ctypes.c_void_p * 4)(pa, pb, pc, None)))
    # n == 0 and H * W == 0 are successful no-ops
    assert batch(0, 2, 2) == 0 and batch(2, 0, 4) == 0 and batch(2, 4, 0) == 0
    assert cfa(H=0) == 0 and raw(W=0) == 0


@pytest.mark.parametrize("cam", ["Camera16", "Camera32"])
def test_loader_rules_are_checked_before_anything_is_uploaded(em, cam):
    """Every rejection happens on host tensors: nothing has touched a device."""
    import taichi_image_amd as ti
    with pytest.raises(ValueError, match="exposure_merge"):
        getattr(ti, cam)(ti.BayerPattern.RGGB, exposure_merge=True)
    s = ti.ExposureMerge((1, 4), GAIN, READ_NOISE)
    on = getattr(ti, cam)(ti.BayerPattern.RGGB, exposure_merge=s)
    off = getattr(ti, cam)(ti.BayerPattern.RGGB)
    assert on.exposure_merge == s and off.exposure_merge is None
    with pytest.raises(AttributeError):
        on.exposure_merge = None
    p12 = torch.zeros((4, 6), dtype=torch.uint8)
    p16 = torch.zeros((4, 8), dtype=torch.uint8)
    u16 = torch.zeros((4, 4), dtype=torch.uint16)
    f = torch.zeros((4, 4), dtype=torch.float32)
    brackets = dict(load_packed12_bracket=[p12, p12], load_packed16_bracket=[p16, p16], load_16u_bracket=[u16, u16],
                    load_16f_bracket=[u16, u16], load_32f_bracket=[f, f], load_packed12_bracket_batch=[[p12, p12]],
                    load_packed16_bracket_batch=[[p16, p16]])
    # a bracket loader while the stage is off
    for name in BRACKET_LOADERS:
        with pytest.raises(ValueError, match="exposure_merge is off"):
            getattr(off, name)(brackets[name])
    # a single-frame loader, or process_packed12, while it is on: the message names the bracket loaders
    for call in (lambda: on.load_packed12(p12), lambda: on.load_packed16(p16), lambda: on.load_16u(u16),
                 lambda: on.load_16f(u16), lambda: on.load_32f(f), lambda: on.load_packed12_batch([p12, p12]),
                 lambda: on.load_packed16_batch([p16]), lambda: on.process_packed12([p12])):
        with pytest.raises(ValueError, match="load_packed12_bracket"):
            call()
    # a bracket whose length is not E
    for name in BRACKET_LOADERS:
        b = brackets[name]
        short = [b[0][:1]] if name.endswith("batch") else b[:1]
        long = [b[0] * 2] if name.endswith("batch") else b * 2
        for v in (short, long):
            with pytest.raises(ValueError, match="ratios"):
                getattr(on, name)(v)
    with pytest.raises(ValueError, match="list"):
        on.load_packed12_bracket(p12)
    with pytest.raises(ValueError, match="list"):
        on.load_packed12_bracket_batch(p12)
    with pytest.raises(ValueError, match="ratios"):
        on.load_packed12_bracket_batch([[p12, p12], [p12]])
    # frames of different shape, dtype or device within a bracket
    with pytest.raises(ValueError, match="share"):
        on.load_packed12_bracket([p12, torch.zeros((6, 6), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="share"):
        on.load_32f_bracket([f, f.double()])
    with pytest.raises(ValueError, match="share"):
        on.load_16u_bracket([u16, torch.zeros((4, 6), dtype=torch.uint16)])
    with pytest.raises(ValueError, match="share"):
        on.load_32f_bracket([f, torch.zeros((4, 4), device="meta")])
    with pytest.raises(ValueError, match="share"):
        on.load_packed16_bracket_batch([[p16, p16], [p12, p12]])             # (brackets of a call share a shape, too)
    with pytest.raises(TypeError):
        on.load_32f_bracket([f, np.zeros((4, 4), f32)])
    # levels with 16f / 32f sources, as today
    lv = getattr(ti, cam)(ti.BayerPattern.RGGB, exposure_merge=s, black_level=[64, 64, 64, 64], white_level=4000)
    for call in (lambda: lv.load_16f_bracket([u16, u16]), lambda: lv.load_32f_bracket([f, f])):
        with pytest.raises(ValueError, match="normalised"):
            call()
    # one defect map per bracket, one history per bracket, and only with temporal noise reduction on
    with pytest.raises(ValueError, match="defects"):
        on.load_packed12_bracket_batch([[p12, p12], [p12, p12]], defects=[None])
    with pytest.raises(ValueError, match="temporal_denoise is off"):
        on.load_packed12_bracket([p12, p12], history=ti.TemporalHistory())
    tn = getattr(ti, cam)(ti.BayerPattern.RGGB, exposure_merge=s, temporal_denoise=ti.TemporalDenoise(GAIN, READ_NOISE))
    with pytest.raises(ValueError, match="history="):
        tn.load_packed12_bracket([p12, p12])
    with pytest.raises(ValueError, match="history="):
        tn.load_packed12_bracket_batch([[p12, p12], [p12, p12]], history=[ti.TemporalHistory()])
    assert on.load_packed12_bracket_batch([]) == []
    # set(): None leaves it, False turns it off, an ExposureMerge replaces it
    on.set(exposure_merge=None)
    assert on.exposure_merge is s
    on.set(exposure_merge=ti.ExposureMerge((1, 2, 4), 0.0, 0.01))
    assert on.exposure_merge.exposures == 3
    with pytest.raises(ValueError, match="ratios"):
        on.load_packed12_bracket([p12, p12])
    with pytest.raises(ValueError, match="exposure_merge"):
        on.set(exposure_merge=True)
    on.set(exposure_merge=False)
    assert on.exposure_merge is None
    with pytest.raises(ValueError, match="exposure_merge is off"):
        on.load_packed12_bracket([p12, p12, p12])
    # merge_cfa's own arguments
    c = np.zeros((4, 4), f32)
    with pytest.raises(ValueError, match="ExposureMerge"):
        em.merge_cfa([c, c], ((1, 4), GAIN, READ_NOISE))
    with pytest.raises(ValueError, match="list of 2"):
        em.merge_cfa([c], s)
    with pytest.raises(ValueError, match="list of 2"):
        em.merge_cfa(c, s)
    with pytest.raises(ValueError, match="f16 or f32"):
        em.merge_cfa([c.astype(np.uint16)] * 2, s)
    with pytest.raises(ValueError, match="differs"):
        em.merge_cfa([c, np.zeros((4, 6), f32)], s)
    with pytest.raises(ValueError, match="differs"):
        em.merge_cfa([c, c.astype(np.float16)], s)
    with pytest.raises(ValueError, match="differs"):
        em.merge_cfa([c, torch.zeros((4, 4))], s)


# ---- the contract on the reference ---------------------------------------------------------------------------------------
def r32(x):
    """The f32 nearest to the Fraction x (ties to even; normal range), as a Fraction."""
    x = Fr(x)
    if x == 0:
        return x
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = 0
    while Fr(2) ** (e + 1) <= x:
        e += 1
    while Fr(2) ** e > x:
        e -= 1
    ulp = Fr(2) ** (e - 23)
    q = x / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fr(1, 2) or (rem == Fr(1, 2) and n % 2 == 1):
        n += 1
    return sign * n * ulp


def test_hand_computed_vector():
    """A 6 x 6 frame, E = 2, ratios (1, 4): inv = 1/4, i2 = 1/16.  gain 0 and read_noise 1/4: v0 = rn2 = 1/16, a0 = 16,
    ve = rn2 i2 = 1/256 for every pixel; threshold 2: c = 4, c (v0 + ve) = 17/64; saturation 1, knee 1/2: rf = 2.
    x_0 = 1/8 and x_1 = 1/2 + e / 16, so se = 1/8 + e / 64 and |se - x_0| = |e| / 64 - except on the even-row, odd-column
    site plane, where x_0 = 1 and x_1 = 0 (something that moved).  Every value is a dyadic rational that f32 holds; the
    operations that round are rounded by r32 above.  (3, 3) is a listed defect."""
    e = np.zeros((6, 6))
    e[0::2, 0::2] = [[2, 1, 0], [0.5, 0.5, 0], [1, 1, 0]]           # the even-even site plane: rows 0, 2, 4 x columns 0, 2, 4
    e[1::2, 1::2] = [[1, -3, 0], [2, 400, 0], [0, 0, 0]]            # the odd-odd one: rows 1, 3, 5 x columns 1, 3, 5
    x0 = np.full((6, 6), 0.125, f32)
    x1 = (0.5 + e / 16).astype(f32)
    x0[0::2, 1::2] = 1.0
    x1[0::2, 1::2] = 0.0
    assert np.array_equal(x1.astype(np.float64), np.where(x0 == 1, 0, 0.5 + e / 16))          # (f32 holds them)
    listed = np.zeros((6, 6), bool)
    listed[3, 3] = True
    s = M.Settings((1, 4), 0.0, 0.25, saturation=1.0, knee=0.5, threshold=2.0)
    assert (s.inv[1], s.i2[1], s.rn2, s.c, s.rf) == (0.25, 0.0625, 0.0625, 4.0, 2.0)
    n, [(u, k, w)] = M.detail([x0, x1], s, listed)
    y = M.merge([x0, x1], s, listed)

    def by_hand(m, xe, s0=Fr(1, 8)):
        """(u, k, w, y) of a pixel with metric m, x_1 = xe and x_0 = s0, every intermediate a Fraction."""
        v0, ve = Fr(1, 16), Fr(1, 256)                       # gain 0: rn2, and rn2 i2
        a0 = 1 / v0                                          # 16
        num, den = a0 * s0, a0                               # 2 (for s0 = 1/8), 16
        qv = r32(r32(m * m) / (4 * (v0 + ve)))               # (m m) / (c (v0 + ve)) = (m m) / (17/64): rounds
        kk = max(r32(1 - qv), 0)                             # rounds
        uu = min(max((1 - xe) * 2, 0), 1)                    # (saturation - x_1) rf: exact here
        ww = r32(uu * kk) / ve                               # u k rounds; / (1/256) is exact
        if ww > 0:
            num = r32(num + r32(ww * (xe / 4)))              # se(p) = x_1 inv
            den = r32(den + ww)
            return uu, kk, ww, r32(num / den)
        return uu, kk, ww, s0

    # the corner (0, 0): taps (0, 0) (0, 2) (2, 0) (2, 2), n = 4, D = (2 + 1 + 1/2 + 1/2) / 64 = 1/16, m = 1/64,
    # m m = 1/4096, qv = r32(1/1088); x_1 = 1/2 + 2/16 = 5/8, inside the knee [1/2, 1): u = 3/4
    uu, kk, ww, yv = by_hand(Fr(1, 64), Fr(5, 8))
    assert uu == Fr(3, 4) and kk == r32(1 - r32(Fr(1, 1088))) and 0 < kk < 1
    assert n[0, 0] == 4 and u[0, 0] == float(uu) and k[0, 0] == float(kk) and w[0, 0] == float(ww) and y[0, 0] == float(yv)
    assert Fr(1, 8) < yv < Fr(1, 8) + Fr(2, 64)              # between x_0 and se = 1/8 + 2/64
    # the edge (2, 0): rows 0, 2, 4 x columns 0, 2, n = 6, D = 6/64; R[6] = 11184811 / 2^26, D R[6] = (2^26 + 2) / 2^32,
    # which rounds to the 24-bit 1/64; x_1 = 1/2 + 1/32: u = 15/16
    assert float(s.R[6]) == 11184811 / 2 ** 26 and r32(Fr(6, 64) * Fr(11184811, 2 ** 26)) == Fr(1, 64)
    uu, kk, ww, yv = by_hand(Fr(1, 64), Fr(17, 32))
    assert uu == Fr(15, 16)
    assert n[2, 0] == 6 and u[2, 0] == float(uu) and k[2, 0] == float(kk) and w[2, 0] == float(ww) and y[2, 0] == float(yv)
    # (1, 1): rows 1, 3 x columns 1, 3 without the listed (3, 3): n = 3, D = (1 + 3 + 2) / 64 = 3/32, m = r32(D R[3]);
    # x_1 = 1/2 + 1/16: u = 7/8
    m = r32(Fr(3, 32) * Fr(float(s.R[3])))
    uu, kk, ww, yv = by_hand(m, Fr(9, 16))
    assert n[1, 1] == 3 and u[1, 1] == float(uu) and k[1, 1] == float(kk) and w[1, 1] == float(ww) and y[1, 1] == float(yv)
    assert yv != Fr(1, 8)
    # with the listed tap counted ((400 + 6) / 64 / 4 = 1.59 standard deviations of 1/4 ... squared over 17/64: qv > 1)
    # the pixel would have kept x_0: a listed defect never feeds a neighbour's metric
    assert M.detail([x0, x1], s)[1][0][1][1, 1] == 0 and M.merge([x0, x1], s)[1, 1] == x0[1, 1]
    # the listed centre (3, 3) is merged like any other pixel, on its eight unlisted taps, from its own values: x_1 = 25.5 is
    # above the saturation, u = 0, and it keeps x_0
    assert n[3, 3] == 8 and u[3, 3] == 0 and w[3, 3] == 0 and y[3, 3] == x0[3, 3]
    # the plane that moved: |se - x_0| = 1 at every tap, m = 1 (n R[n] rounds to 1 for n = 4, 6, 9 alike), qv = 64/17 > 1:
    # k = 0 although the long frame is fully usable (u = 1), and y = x_0 bit for bit
    uu, kk, ww, yv = by_hand(Fr(1), Fr(0), Fr(1))
    assert (uu, kk, ww, yv) == (1, 0, 0, 1)
    assert np.all(u[0::2, 1::2] == 1) and np.all(k[0::2, 1::2] == 0) and np.array_equal(y[0::2, 1::2], x0[0::2, 1::2])
    # every other pixel has se == x_0: m = 0, k = 1, u = 1, w = 256, num = 2 + 256 / 8 = 34, den = 272, y = 1/8
    assert w[1, 0] == 256 and k[1, 0] == 1 and np.array_equal(y[1::2, 0::2], x0[1::2, 0::2])


def test_a_pixel_without_taps_keeps_x0():
    x0 = np.array([[0.25, 0.5], [0.75, 0.125]], f32)
    x1 = (x0 * f32(2)).astype(f32)
    listed = np.array([[True, False], [False, False]])
    s = M.Settings((1, 2), 0.0, 0.25, saturation=4.0)
    n, [(u, k, w)] = M.detail([x0, x1], s, listed)
    assert n[0, 0] == 0 and w[0, 0] > 0                      # (m = 0, so k = 1: the weights alone would merge it)
    y = M.merge([x0, x1], s, listed)
    assert y[0, 0] == x0[0, 0]
    assert np.array_equal(y, x0)                             # (the others: se == x_0, merged to the same value)
    x1[0, 0] = 0.4                                           # ... whatever the long frame holds there
    assert M.merge([x0, x1], s, listed)[0, 0] == x0[0, 0]
    assert M.merge([x0, x1], s)[0, 0] != x0[0, 0]


@pytest.mark.parametrize("E", [2, 3, 4])
def test_exact_property_saturated_long_frames(rng, E):
    """Where every long frame is at or above the saturation, y = x_0 bit for bit."""
    H, W = 34, 38
    s = M.Settings(RATIOS[E], GAIN, READ_NOISE)
    x0 = rng.random((H, W)).astype(f32)
    frames = [x0] + [np.maximum(f32(s.sat), rng.random((H, W)).astype(f32) * f32(1.2)).astype(f32) for _ in range(E - 1)]
    frames[1][0, 0] = s.sat                                  # (at the saturation exactly)
    assert np.array_equal(M.merge(frames, s), x0)
    frames[1][10:20, 10:20] = (x0[10:20, 10:20] * f32(0.1) * f32(RATIOS[E][1])).astype(f32)
    y = M.merge(frames, s)
    inside = np.zeros((H, W), bool)
    inside[10:20, 10:20] = True
    assert np.array_equal(y[~inside], x0[~inside])           # (a pixel's own values decide u: the window does not)


@pytest.mark.parametrize("E", [2, 3, 4])
def test_exact_property_motion_leaves_no_ghost(rng, E):
    """Where every long frame's window differs from the shortest by more than `threshold` standard deviations (qv > 1),
    y = x_0 bit for bit, although every long frame is fully usable there."""
    H, W = 34, 38
    ratios = RATIOS[E]
    s = M.Settings(ratios, GAIN, READ_NOISE)
    x0 = (0.002 + 0.01 * rng.random((H, W))).astype(f32)
    sigma = np.sqrt(GAIN * 0.03 + READ_NOISE ** 2)           # (above the model's sigma of both frames together)
    frames = [x0] + [((x0 + f32(4.5 * 2 * sigma)) * f32(q)).astype(f32) for q in ratios[1:]]
    n, per = M.detail(frames, s)
    assert all(np.all(u == 1) and np.all(k == 0) for u, k, _ in per)
    assert np.array_equal(M.merge(frames, s), x0)
    # ... and a difference of one standard deviation is merged
    frames = [x0] + [((x0 + f32(sigma)) * f32(q)).astype(f32) for q in ratios[1:]]
    assert np.all(M.merge(frames, s) != x0)


def test_noise_on_a_static_scene():
    """A smooth 128 x 128 scene over [0.002, 0.8] with noise drawn from the model, ratios (1, 4, 16), 32 brackets: the
    residual noise power of y in the dark third of the scene (by clean value) against that of the shortest frame alone.
    Measured with this seed: 0.0157 (the mid-tone third, where the longest frame saturates: 0.028); asserted with a
    25 % margin for the seed's spread."""
    rng = np.random.default_rng(1234)
    scene = M.smooth_scene(128, 128)
    ratios = (1, 4, 16)
    s = M.Settings(ratios, GAIN, READ_NOISE)
    dark = scene <= np.quantile(scene, 1 / 3)
    mid = (scene > np.quantile(scene, 1 / 3)) & (scene <= np.quantile(scene, 2 / 3))
    acc = np.zeros(4)
    for _ in range(32):
        frames = M.static_bracket(rng, scene, ratios, GAIN, READ_NOISE)
        y = M.merge(frames, s).astype(np.float64)
        ey, e0 = (y - scene) ** 2, (frames[0] - scene) ** 2
        acc += [ey[dark].sum(), e0[dark].sum(), ey[mid].sum(), e0[mid].sum()]
    ratio_dark, ratio_mid = acc[0] / acc[1], acc[2] / acc[3]
    print(f"residual noise power: dark third {ratio_dark:.4f}, mid-tone third {ratio_mid:.4f}")
    assert ratio_dark < 0.0157 * 1.25
    assert ratio_mid < 0.028 * 1.25
    # inverse-variance weights cannot do better than the sum of the frames' precisions
    assert ratio_dark > 1 / (1 + 16 + 256)


def test_a_moved_block_leaves_no_ghost():
    """A bright block that is in the shortest frame and not in the long ones (it moved between the exposures): every pixel at
    least 2 columns and rows inside the block equals x_0 bit for bit, and the rest of the scene is merged."""
    rng = np.random.default_rng(77)
    H, W = 64, 64
    ratios = (1, 4, 16)
    s = M.Settings(ratios, GAIN, READ_NOISE)
    scene = 0.01 + 0.02 * M.smooth_scene(H, W, 0.1, 1.0)
    with_block = scene.copy()
    with_block[20:44, 24:48] = 0.15
    frames = [M.expose(rng, with_block, 1, GAIN, READ_NOISE).astype(f32)]
    frames += [M.expose(rng, scene, q, GAIN, READ_NOISE).astype(f32) for q in ratios[1:]]
    y = M.merge(frames, s)
    assert np.array_equal(y[22:42, 26:46], frames[0][22:42, 26:46])
    outside = np.ones((H, W), bool)
    outside[18:46, 22:50] = False
    assert (y != frames[0])[outside].mean() > 0.95
    # the long frames are usable there: it is the metric that drops them
    _, per = M.detail(frames, s)
    assert np.all(per[0][0][22:42, 26:46] == 1) and np.all(per[0][1][22:42, 26:46] == 0)


@pytest.mark.parametrize("E", [2, 3, 4])
@pytest.mark.parametrize("H,W", [(64, 64), (66, 70), (130, 66)])
def test_the_generated_brackets_exercise_the_operator(rng, H, W, E):
    """make_bracket on the reference alone: at least 10 % of the pixels in each of the four classes - shortest only because
    the long frames are saturated; shortest only because they were rejected; some long frame inside its knee; every long
    frame fully usable - also after the 12-bit quantisation of the packed loaders."""
    ratios = RATIOS[E]
    s = M.Settings(ratios, GAIN, READ_NOISE)
    us = M.make_bracket(rng, H, W, ratios, GAIN, READ_NOISE)
    for frames in ([u.astype(f32) for u in us], [(np.rint(u * 4095) / 4095).astype(f32) for u in us]):
        shares = M.classes(frames, s)
        assert min(shares) >= 0.10, shares
        y = M.merge(frames, s)
        assert 0.3 < (y != frames[0]).mean() < 0.7


def test_the_rounding_bracket_tells_the_orders_apart(rng):
    """On rounding_bracket the reversed tap order and the reversed exposure order each change a share of the pixels
    (measured at 66 x 70: 28 % and 27 %)."""
    for H, W in [(66, 70), (130, 66)]:
        frames, args = M.rounding_bracket(rng, H, W)
        y = M.merge(frames, args)
        taps = (y != M.merge(frames, args, taps=M.TAPS[::-1])).mean()
        order = (y != M.merge(frames, args, order=[2, 1])).mean()
        print(f"{H}x{W}: reversed taps change {taps:.3f}, reversed exposures {order:.3f}")
        assert taps > 0.05 and order > 0.05
        _, per = M.detail(frames, args)
        assert all(((k > 0) & (k < 1)).mean() > 0.8 for _, k, _ in per)
