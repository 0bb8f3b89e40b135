"""The C/OpenMP restatement (oracle/isp_oracle.c) against the NumPy restatement: two independent
implementations of the same specification must agree -- bit-exactly for unpack, f16 rounding and
demosaic, within the fp tolerance for the libm-dependent tonemap."""
import numpy as np
import pytest

from oracle import c_oracle, isp_oracle as O
from tests.util import (DEGENERATE, GAMMAS, assert_close, assert_exact, degenerate_cfa, nan_on_grid, natural_packed12,
                        scene_cut_frames, scene_cut_state)

pytestmark = pytest.mark.skipif(not c_oracle.available(), reason="oracle/liborc_isp.so not built (run build())")


def test_tables_and_f16_rounding(rng):
    assert np.array_equal(c_oracle.bayer_kernels(), O.BAYER_KERNELS)
    x = np.concatenate([rng.random(20000, dtype=np.float32) * 2 - 1, (rng.random(2000) * 1e-4).astype(np.float32),
                        (rng.random(2000) * 1e-7).astype(np.float32),
                        np.array([0, 1, 65504, 65519.9, 65520, 1e6, 2.0 ** -24, 2.0 ** -25, 6.1e-5, np.inf, -np.inf], np.float32)])
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    got = np.array([c_oracle.lib().orc_f32_to_f16_bits(float(v)) for v in x], np.uint16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("ids", [False, True])
def test_decode12(rng, ids):
    enc = rng.integers(0, 256, 3 * 4001).astype(np.uint8)
    for work in ("f16", "f32"):
        assert_exact(c_oracle.decode12_scaled(enc, ids, work), O.decode12(enc, work, True, ids).astype(np.float32))


@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_demosaic_bit_exact(rng, p):
    cfa = rng.random((38, 54), dtype=np.float32)
    assert_exact(c_oracle.demosaic(cfa, p), O.bayer_to_rgb(cfa, p))
    h = cfa.astype(np.float16)
    assert_exact(c_oracle.demosaic(h.astype(np.float32), p, round_f16=True).astype(np.float16), O.bayer_to_rgb(h, p))
    ccm = O.isp_color_matrix(True, O.DEFAULT_WB, O.DEFAULT_CC)
    assert_exact(c_oracle.demosaic(cfa, p, ccm=ccm), O.bayer_to_rgb(cfa, p, ccm))
    u16 = rng.integers(0, 65536, (12, 20)).astype(np.uint16)
    got = c_oracle.demosaic(u16.astype(np.float32), p, in_scale=65535.0)
    assert_exact(O.cast_out(got * np.float32(65535), "u16"), O.bayer_to_rgb(u16, p))


@pytest.mark.parametrize("out", ["f16", "u8", "f32"])
@pytest.mark.parametrize("kw", [dict(), dict(gamma=0.6, intensity=1.5, light_adapt=0.7, color_adapt=0.4)])
def test_pipeline(rng, out, kw):
    packed = natural_packed12(rng, 64, 96)
    work = "f32" if out == "f32" else "f16"
    got = c_oracle.pipeline12_reinhard(packed, work=work, out=out, **kw)
    assert_close(got, O.pipeline12_reinhard(packed, work=work, out=out, **kw), f"C vs NumPy pipeline {out}")


@pytest.mark.parametrize("work", ["f16", "f32"])
def test_isp_stateful_path(rng, work):
    """camera_isp.py:142-227 in C against the NumPy restatement: the 9-vector over three steps (moving
    average), the u8 outputs and the in-place write-back of Reinhard, the linear map."""
    st_c, st_n = c_oracle.IspState(0.3), O.IspState(0.3)
    for step in range(3):
        imgs = [O.isp_load_packed12(natural_packed12(rng, 80, 96, dark=0.05 * step), work) for _ in range(3)]
        mc, mn = st_c.update_metering(imgs), st_n.update_metering(imgs)
        assert_close(mc, mn, f"metering step {step}", rel=2e-6)
        for kw in (dict(gamma=0.6), dict(gamma=1.0, intensity=0.7, light_adapt=0.8, color_adapt=0.3)):
            for im in imgs:
                u8_c, after_c = c_oracle.reinhard_isp(im, mn, **kw)
                u8_n, after_n = O.reinhard_isp(im, mn, **kw)
                assert_close(u8_c, u8_n, "reinhard u8")
                assert_close(after_c, after_n, "reinhard write-back")
        assert_close(c_oracle.linear_isp(imgs[0], mn, 0.8), O.linear_isp(imgs[0], mn, 0.8), "linear")


# ---- the edges: what the smooth in-range scenes above never produce ------------------------------------------------

@pytest.mark.parametrize("work", ["f16", "f32"])
def test_metering_nan_inf_and_out_of_range(rng, work):
    """The NaN rule of the module docstring of oracle/isp_oracle.py: min / max (the bounds, the max(gray, 1e-4) clamp, the
    log bounds) ignore NaN, sums propagate it.  NaN on the stride-8 grid (first and last sample), +-inf and values outside
    [0, 1], with a fresh state and blended into a previous one."""
    dt = np.float16 if work == "f16" else np.float32
    base = O.isp_load_packed12(natural_packed12(rng, 64, 72), work).astype(np.float32)
    nan1 = nan_on_grid(base)
    assert np.isnan(nan1[::8, ::8]).any(), "no NaN on the metering grid"
    out_of_range = base * 1.6 - 0.3
    assert (out_of_range[::8, ::8] < 0).any() and (out_of_range[::8, ::8] > 1).any()
    inf = np.array(base, copy=True)
    inf[8, 16, 0] = np.inf
    ninf = np.array(base, copy=True)
    ninf[16, 8, 2] = -np.inf
    all_nan = np.full_like(base, np.nan)
    prev = np.array([0.05, 0.9, -5.0, -0.1, -1.2, 0.45, 0.5, 0.45, 0.4], np.float32)
    for name, imgs in [("nan", [nan1]), ("nan+clean", [base, nan1]), ("out of range", [out_of_range]),
                       ("+inf", [inf]), ("-inf", [ninf]), ("all nan", [all_nan, base])]:
        ims = [im.astype(dt) for im in imgs]
        for alpha, pv in ((0.0, np.zeros(9, np.float32)), (0.7, prev)):
            got, want = c_oracle.metering_images(ims, alpha, pv), O.metering_images(ims, alpha, pv)
            assert_close(got, want, f"metering {name} alpha {alpha}", rel=2e-6)
    # the rule itself, on the NaN frame: bounds and log bounds finite, the green mean and the gray mean NaN
    for m in (O.metering_images([nan1.astype(dt)], 0.0, np.zeros(9, np.float32)),
              c_oracle.metering_images([nan1.astype(dt)], 0.0, np.zeros(9, np.float32))):
        assert np.isfinite(m[:5]).all() and np.isfinite(m[[6, 8]]).all(), m
        assert np.isnan(m[5]) and np.isnan(m[7]), m
        # the bounds are those of the subsample with the NaN sites removed
        sub = nan1.astype(dt)[::8, ::8].astype(np.float32)
        clean = sub[~np.isnan(sub)]
        assert m[0] == clean.min() and m[1] == clean.max(), (m[:2], clean.min(), clean.max())


@pytest.mark.parametrize("bright", [True, False])
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("la,ca", [(1.0, 0.0), (0.6, 0.4)])
def test_scene_cut_reinhard_and_linear(bright, gamma, la, ca):
    """Pixels outside the metering bounds (a scene cut against the previous state) through reinhard_isp and linear_isp,
    with integral (2, 4, 3, 1) and non-integral 1/gamma: powf of a negative base is defined for an integral exponent."""
    rng = np.random.default_rng(11)
    st_n, st_c = O.IspState(0.3), c_oracle.IspState(0.3)
    st_n.metrics = scene_cut_state(rng, 48, 64, bright)
    st_c.metrics = st_n.metrics.copy()
    imgs = [O.isp_load_packed12(f, "f16") for f in scene_cut_frames(rng, 48, 64, bright)]
    mn, mc = st_n.update_metering(imgs), st_c.update_metering(imgs)
    assert_close(mc, mn, "metering", rel=2e-6)
    sc = (np.stack(imgs).astype(np.float32) - mn[0]) / (mn[1] - mn[0])
    assert (sc < 0).any() if bright else (sc > 1).any(), "the scene cut leaves every pixel inside the bounds"
    for im in imgs:
        u8_c, after_c = c_oracle.reinhard_isp(im, mn, gamma=gamma, light_adapt=la, color_adapt=ca)
        u8_n, after_n = O.reinhard_isp(im, mn, gamma=gamma, light_adapt=la, color_adapt=ca)
        assert_close(u8_c, u8_n, "reinhard u8")
        assert_close(after_c, after_n, "reinhard write-back")
        lin_c, lin_n = c_oracle.linear_isp(im, mn, gamma), O.linear_isp(im, mn, gamma)
        assert_close(lin_c, lin_n, "linear")
    below = (imgs[0].astype(np.float32) < mn[0])
    lin = O.linear_isp(imgs[0], mn, gamma)
    if bright and np.float32(1) / np.float32(gamma) in (2.0, 4.0):
        # even exponent: (x - lo)^e > 0 below the bounds - what exp2(e log2 b) (NaN -> 0) got wrong
        assert (lin[below] > 0).any(), "no pixel below the bounds maps to a nonzero u8"
    else:
        assert (lin[below] == 0).all()
    if la < 1 and bright:
        _, after = O.reinhard_isp(imgs[0], mn, gamma=gamma, light_adapt=la, color_adapt=ca)
        assert (after.astype(np.float32) < 0).any(), "no p < 0"


@pytest.mark.parametrize("kind", DEGENERATE)
@pytest.mark.parametrize("out", ["f16", "u8"])
def test_degenerate_frames_pipeline(kind, out):
    """hi == lo (inv = inf, 0 * inf = NaN, key = 0/0), bounds exactly (0, 1), a single non-black pixel."""
    packed = O.encode12(degenerate_cfa(kind, 26, 40))
    kw = dict(gamma=0.5, light_adapt=0.6, color_adapt=0.4)
    for k in (dict(), kw):
        got = c_oracle.pipeline12_reinhard(packed, out=out, **k)
        want = O.pipeline12_reinhard(packed, out=out, **k)
        if kind in ("zero", "full", "flat"):
            assert_exact(got, want, f"{kind} {out} {k}")
            assert not np.any(want.astype(np.float32)), "a flat frame maps to zero"
        else:
            assert_close(got, want, f"{kind} {out} {k}")


def test_degenerate_metering_state_recovers():
    """Flat frames (hi == lo) inside a rolling sequence: the two restatements agree on the state and the outputs at every
    step, and the state is finite again once the scene returns."""
    rng = np.random.default_rng(3)
    st_n, st_c = O.IspState(0.3), c_oracle.IspState(0.3)
    seq = ["scene", "zero", "full", "flat", "scene", "scene"]
    for step, kind in enumerate(seq):
        if kind == "scene":
            frames = [natural_packed12(rng, 32, 48, dark=0.05 * k) for k in range(2)]
        else:
            frames = [O.encode12(degenerate_cfa(kind, 32, 48))] * 2
        imgs = [O.isp_load_packed12(f, "f16") for f in frames]
        mn, mc = st_n.update_metering(imgs), st_c.update_metering(imgs)
        assert_close(mc, mn, f"metering step {step} ({kind})", rel=2e-6)
        for im in imgs:
            assert_close(c_oracle.reinhard_isp(im, mn, gamma=0.5)[0], O.reinhard_isp(im, mn, gamma=0.5)[0], f"u8 {step}")
            assert_close(c_oracle.linear_isp(im, mn, 0.5), O.linear_isp(im, mn, 0.5), f"linear {step}")
    assert np.isfinite(st_n.metrics).all(), st_n.metrics
