"""GPU parity at the edges every other test stays away from: pixels outside the metering bounds after a scene cut (p < 0,
negative bases under an integral 1/gamma), degenerate frames (hi == lo: inv = inf, 0 * inf = NaN, key = 0/0; bounds
exactly (0, 1)), NaN on the metering subsample (the p = NaN the ISP Reinhard writes back over black pixels with
light_adapt == 1), and single pixels that decide a bound or max_out at the edges of the kernels' decompositions.

Every case checks its own premise through the oracle: that the situation under test occurs at all."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, isp_oracle as O
from tests.util import (DEGENERATE, GAMMAS, assert_close, degenerate_cfa, natural_packed12, scene_cut_frames,
                        scene_cut_state)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not c_oracle.available(), reason="oracle/liborc_isp.so not built")]


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _seeded(ti, dev, cam, state, alpha=0.3, **kw):
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=alpha, device=dev, **kw)
    isp.metrics = torch.from_numpy(np.array(state, np.float32)).to(dev)
    st = c_oracle.IspState(alpha)
    st.metrics = np.array(state, np.float32)
    return isp, st


def _host(t):
    return t.cpu().numpy()


def _p_rel(img, m, light_adapt=1.0, color_adapt=0.0, **_):
    """Per-value relative tolerance of the stored p = sc / (ad + sc), ad = (e^-i am)^map_key (camera_isp.py:200-210): the
    contract's 1e-4 plus a first-order propagation of a few f32 ulps (2^-20 relative: the hardware log / exp / rcp, a fused
    or unfused multiply-add) through the two places the formula is ill-conditioned - the pole ad + sc = 0, which pixels
    below the bounds reach when light_adapt < 1, and am -> 0, where d ad / d am = map_key ad / am grows without bound."""
    eps = 2.0 ** -20
    bmin, bmax, map_key, mean3 = O.reinhard_params(m, 1.0, light_adapt, color_adapt)
    la, ca = np.float32(light_adapt), np.float32(color_adapt)
    with np.errstate(all="ignore"):
        sc = (img.astype(np.float32) - bmin) / (bmax - bmin)
        g = (sc[..., 0] * O.GRAY_W[0] + sc[..., 1] * O.GRAY_W[1] + sc[..., 2] * O.GRAY_W[2])[..., None]
        ac = g + ca * (sc - g)
        am = mean3 + la * (ac - mean3)
        ad = np.power(np.float32(np.exp(-1.0)) * am, map_key)
        err_am = eps * (np.abs(mean3) + la * (np.abs(ac) + np.abs(mean3) + np.abs(g) + np.abs(sc)))
        err_ad = np.abs(ad) * (eps + np.abs(map_key) * err_am / np.abs(am))
        rel = 1e-4 + (err_ad + eps * np.abs(sc)) / np.abs(ad + sc)
    return np.nan_to_num(rel, nan=1e-4, posinf=1e-4)


def _u8_rel(img, m, ref_after, gamma, **kw):
    """Relative tolerance of the Reinhard u8 output 255 (p / max_out)^(1/gamma): max_out is one p, and when that p lies
    next to the pole its error (_p_rel) scales the whole image - by (1/gamma) times its relative error."""
    a = ref_after.astype(np.float32)
    if not np.isfinite(a).any():
        return 1e-4
    i = np.unravel_index(np.nanargmax(np.where(np.isinf(a), np.nan, a)), a.shape)
    return 1e-4 + float(_p_rel(img, m, **kw)[i]) / gamma


# ---- A. pixels outside the metering bounds (scene cuts) ------------------------------------------------------------

def _bits(t):
    """Bit view for torch.equal (p holds NaN over black pixels, and -0 != +0)."""
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _scene_cut_premise(refs, m, bright, gamma, la, ca):
    sc = (np.stack(refs).astype(np.float32) - m[0]) / (m[1] - m[0])
    if not bright:
        assert (sc > 1).any(), "no pixel above the bounds"
        return
    assert (sc < 0).any(), "no pixel below the bounds"
    e = np.float32(1) / np.float32(gamma)
    res = [c_oracle.reinhard_isp(r, m, gamma=gamma, light_adapt=la, color_adapt=ca) for r in refs]
    if la < 1:
        assert any((after.astype(np.float32) < 0).any() for _, after in res), "no p < 0"
    if e in (2.0, 4.0):
        # where powf and exp2(e log2 b) (NaN -> 0) part: a base below the bounds with a visible u8 under powf
        lin = c_oracle.linear_isp(refs[0], m, gamma)
        assert (lin[refs[0].astype(np.float32) < m[0]] > 1).any(), "no pixel below the bounds maps to a visible u8"
        n = sum(int(((after.astype(np.float32) < 0) & (u8 > 1)).sum()) for u8, after in res)
        assert n > 0, "no p < 0 that the Reinhard output maps to a visible u8"


@pytest.mark.parametrize("cam", ["Camera16", "Camera32"])
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("bright", [True, False], ids=["bright_state", "dark_state"])
@pytest.mark.parametrize("shape", [(100, 1032), (96, 1024)], ids=["partial_bands", "whole_waves"])
def test_scene_cut(ti, dev, cam, gamma, bright, shape):
    """A dark group after the state of a bright one (and the reverse) through the ISP tonemaps: Reinhard in two launches,
    write_back=False, process_packed12 with and without the images, and linear - each against the C oracle (powf of the
    negative bases below the bounds), and every Reinhard path bit for bit against the two launches."""
    H, W = shape
    rng = np.random.default_rng(40 + GAMMAS.index(gamma))
    state = scene_cut_state(rng, H, W, bright, "f16" if cam == "Camera16" else "f32")
    frames = [torch.from_numpy(f).to(dev) for f in scene_cut_frames(rng, H, W, bright)]
    paths = ["two_launches", "keep", "process", "process_keep", "linear"]
    for la, ca in ((1.0, 0.0), (0.6, 0.4)):
        kw = dict(gamma=gamma, light_adapt=la, color_adapt=ca)
        two = None
        for path in paths:
            if path == "linear" and la != 1.0:
                continue                            # (no light_adapt / color_adapt in the linear map)
            isp, st = _seeded(ti, dev, cam, state)
            if path.startswith("process"):
                res = isp.process_packed12(frames, keep_images=path == "process_keep", **kw)
                outs, imgs = res if path == "process_keep" else (res, None)
                refs = [O.isp_load_packed12(_host(f), "f16" if cam == "Camera16" else "f32") for f in frames]
            else:
                imgs = [isp.load_packed12(f) for f in frames]
                refs = [_host(im) for im in imgs]
                if path == "linear":
                    outs = isp.tonemap_linear(imgs, gamma=gamma)
                else:
                    outs = isp.tonemap_reinhard(imgs, write_back=path != "keep", **kw)
            m = st.update_metering(refs)
            dm = _host(isp.metrics)
            assert_close(dm, m, f"{path} metrics", rel=2e-5)
            _scene_cut_premise(refs, m, bright, gamma, la, ca)
            # (the tonemap's references from the library's state: next to the pole of p the 2e-5 the two states may
            # differ by is amplified like any other error)
            for k in range(len(frames)):
                if path == "linear":
                    assert_close(_host(outs[k]), c_oracle.linear_isp(refs[k], dm, gamma), f"linear img {k}")
                    continue
                ref_u8, ref_after = c_oracle.reinhard_isp(refs[k], dm, **kw)
                assert_close(_host(outs[k]), ref_u8, f"{path} la {la} u8 img {k}", rel=_u8_rel(refs[k], dm, ref_after, **kw))
                if path == "keep":
                    assert np.array_equal(_host(imgs[k]).view(np.uint8), refs[k].view(np.uint8)), "write_back=False wrote"
                elif imgs is not None:
                    assert_close(_host(imgs[k]), ref_after, f"{path} la {la} p img {k}", rel=_p_rel(refs[k], dm, **kw))
            if path == "two_launches":
                two = (isp.metrics.clone(), [o.clone() for o in outs], [im.clone() for im in imgs])
            elif path != "linear":
                # the same state and the same bits as the two launches
                assert torch.equal(isp.metrics, two[0]), f"{path}: metrics differ from the two launches"
                for k in range(len(frames)):
                    assert torch.equal(outs[k], two[1][k]), f"{path} la {la}: u8 img {k} differs from the two launches"
                    if imgs is not None and path != "keep":
                        assert torch.equal(_bits(imgs[k]), _bits(two[2][k])), f"{path} la {la}: p img {k} differs"
        assert two is not None


@pytest.mark.parametrize("gamma", [0.5, 1.0 / 3.0, 0.6])
def test_scene_cut_yuv420_and_resize(ti, dev, gamma):
    """The fused YUV pass (W % 16 == 0) against the conversion of the u8 Reinhard output, and a resize_width camera."""
    rng = np.random.default_rng(7)
    H, W = 36, 528
    state = scene_cut_state(rng, H, W, True)
    frames = [torch.from_numpy(f).to(dev) for f in scene_cut_frames(rng, H, W, True)]
    kw = dict(gamma=gamma, light_adapt=0.6, color_adapt=0.4)
    isp, st = _seeded(ti, dev, "Camera16", state)
    imgs = [isp.load_packed12(f) for f in frames]
    refs = [_host(im) for im in imgs]
    yuv = isp.tonemap_reinhard_yuv420(imgs, **kw)
    m = st.update_metering(refs)
    assert_close(_host(isp.metrics), m, "metrics", rel=2e-5)
    _scene_cut_premise(refs, m, True, gamma, 0.6, 0.4)
    isp2, _ = _seeded(ti, dev, "Camera16", state)
    imgs2 = [isp2.load_packed12(f) for f in frames]
    rgb = isp2.tonemap_reinhard(imgs2, **kw)
    dm = _host(isp.metrics)
    for k in range(len(frames)):
        ref_u8, ref_after = c_oracle.reinhard_isp(refs[k], dm, **kw)
        assert_close(_host(rgb[k]), ref_u8, f"rgb img {k}", rel=_u8_rel(refs[k], dm, ref_after, **kw))
        assert_close(_host(yuv[k]), O.rgb_yuv420(_host(rgb[k])), f"yuv img {k}")
    # resize_width: the loader resizes, the tonemaps see pixels outside the bounds the same way
    isp3, st3 = _seeded(ti, dev, "Camera16", state, resize_width=264)
    imgs3 = [isp3.load_packed12(f) for f in frames]
    refs3 = [_host(im) for im in imgs3]
    outs3 = isp3.tonemap_reinhard(imgs3, **kw)
    m3 = st3.update_metering(refs3)
    assert_close(_host(isp3.metrics), m3, "resize metrics", rel=2e-5)
    _scene_cut_premise(refs3, m3, True, gamma, 0.6, 0.4)
    for k in range(len(frames)):
        dm3 = _host(isp3.metrics)
        ref_u8, ref_after = c_oracle.reinhard_isp(refs3[k], dm3, **kw)
        assert_close(_host(outs3[k]), ref_u8, f"resize img {k}", rel=_u8_rel(refs3[k], dm3, ref_after, **kw))


def _pole_state(v, la):
    """A metering state that puts the grey value v (below bmin) next to the pole of p = sc / (ad + sc), on the side where
    p -> -inf: bmin bisected (in f32) until the oracle's f32 p lies in [-3e6, -2e5] - beyond the f16 range (65504) by a
    margin that absorbs the hardware's error (~|p| * a few ulps relative), short of where that error could flip the sign."""
    m = np.array([0.2, 0.9, -5.0, -0.1, -1.2, 0.45, 0.45, 0.45, 0.45], np.float32)

    def p_at(bmin):
        mm = m.copy()
        mm[0] = bmin
        return float(c_oracle.reinhard_isp(np.full((1, 1, 3), v, np.float32), mm, light_adapt=la)[1][0, 0, 0])
    lo, hi = np.float32(0.13), np.float32(0.4)       # p(lo) slightly < 0, p(hi) NaN (the adaptation base < 0)
    for _ in range(100):
        mid = np.float32((float(lo) + float(hi)) / 2)
        p = p_at(mid)
        if -3e6 <= p <= -2e5:
            m[0] = mid
            return m
        if p < 0:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no bmin puts the value next to the pole")


@pytest.mark.parametrize("cam", ["Camera16", "Camera32"])
def test_p_overflows_next_to_the_pole(ti, dev, cam):
    """A stored p beyond the f16 range (-> -inf in a Camera16 image), which max_out must ignore and the gamma curve then
    maps: powf(-inf, 2) = inf -> 255, powf(-inf, 3) = -inf -> 0.  For a non-integral 1/gamma powf(-inf, e) = +inf -> 255,
    where the library gives NaN -> 0 (not followed, it would cost every value a compare and a select); that
    one value is asserted as the library defines it, everything else against the oracle.  The static reinhard_kernel
    with the state given, so that the library and the oracle use the same metering bits."""
    la, v = 0.6, 0.125
    m = _pole_state(v, la)
    rng = np.random.default_rng(3)
    dt = np.float16 if cam == "Camera16" else np.float32
    img = (0.4 + 0.4 * rng.random((32, 64, 1)) * np.ones(3)).astype(dt)
    img[17, 41] = v
    metrics = torch.from_numpy(m).to(dev)
    for gamma in (0.5, 1.0 / 3.0, 0.6):
        ref_u8, ref_after = c_oracle.reinhard_isp(img, m, gamma=gamma, light_adapt=la)
        p = ref_after[17, 41].astype(np.float32)
        if cam == "Camera16":
            assert np.all(p == -np.inf), f"premise: the stored p does not overflow ({p})"
        else:
            assert np.all(p < -65504), f"premise: p is within the f16 range ({p})"
        even = np.float32(1) / np.float32(gamma) == 2.0
        if cam == "Camera16" and gamma == 0.6:
            assert np.all(ref_u8[17, 41] == 255), ref_u8[17, 41]
            ref_u8 = ref_u8.copy()
            ref_u8[17, 41] = 0                    # powf(-inf, 1.667) = +inf; the library: NaN -> 0 (see the docstring)
        assert np.all(ref_u8[17, 41] == (255 if even else 0)), ref_u8[17, 41]
        im = torch.from_numpy(img).to(dev)
        out = torch.empty((32, 64, 3), dtype=torch.uint8, device=dev)
        getattr(ti, cam).reinhard_kernel(im, out, metrics, gamma, 1.0, la, 0.0)
        assert_close(_host(out), ref_u8, f"u8 gamma {gamma}")
        assert_close(_host(im), ref_after, f"p gamma {gamma}", rel=_p_rel(img, m, light_adapt=la))


@pytest.mark.parametrize("gamma", [0.5])
def test_scene_cut_camera_group_full_size(ti, dev, gamma):
    """4096 x 3072: the camera-group kernel (one persistent launch) with a seeded bright state and a dark group."""
    rng = np.random.default_rng(9)
    H, W = 3072, 4096
    state = scene_cut_state(np.random.default_rng(1), 256, 512, True)
    frames = [torch.from_numpy(f).to(dev) for f in scene_cut_frames(rng, H, W, True, n=1)]
    isp, st = _seeded(ti, dev, "Camera16", state)
    with torch.cuda.device(dev):
        assert ti._native.lib().mi_isp_camera_group_fits(H, W, 0, ti.types.f16.code, 8), "the group takes the two calls"
    kw = dict(gamma=gamma, light_adapt=1.0, color_adapt=0.0)
    outs, imgs = isp.process_packed12(frames, keep_images=True, **kw)
    refs = [O.isp_load_packed12(_host(f), "f16") for f in frames]
    m = st.update_metering(refs)
    dm = _host(isp.metrics)
    assert_close(dm, m, "metrics", rel=2e-5)
    _scene_cut_premise(refs, m, True, gamma, 1.0, 0.0)
    for k in range(len(frames)):
        ref_u8, ref_after = c_oracle.reinhard_isp(refs[k], dm, **kw)
        assert_close(_host(outs[k]), ref_u8, f"u8 img {k}", rel=_u8_rel(refs[k], dm, ref_after, **kw))
        assert_close(_host(imgs[k]), ref_after, f"p img {k}", rel=_p_rel(refs[k], dm, **kw))


# ---- B. degenerate frames ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", DEGENERATE)
@pytest.mark.parametrize("shape", [(26, 520), (130, 1544)])
def test_degenerate_pipeline(ti, dev, kind, shape):
    """All 0, all 4095, flat 1800, binary 0/4095 (bounds exactly (0, 1): the fast path) and one non-black pixel through
    the whole-frame kernel and the multi-pass chain, f16 and u8 out."""
    from taichi_image_amd.pipeline import pipeline12_reinhard
    packed = O.encode12(degenerate_cfa(kind, *shape))
    for kw in (dict(), dict(gamma=0.5, light_adapt=0.6, color_adapt=0.4)):
        for out in ("f16", "u8"):
            want = c_oracle.pipeline12_reinhard(packed, out=out, **kw)
            if kind in ("zero", "full", "flat"):
                assert not np.any(want.astype(np.float32)), "a flat frame maps to zero"
            for wf in (True, False):
                got = _host(pipeline12_reinhard(torch.from_numpy(packed).to(dev), dtype=getattr(ti.types, out),
                                                whole_frame=wf, check=True if wf else None, **kw))
                assert_close(got, want, f"{kind} {out} whole_frame={wf} {kw}")
        # f32 work dtype: still the stream route where the f16 call took it (strm::supported takes f32; the tile routes
        # have tests/test_gpu_multi_pass_matrix.py)
        got = _host(pipeline12_reinhard(torch.from_numpy(packed).to(dev), work_dtype=ti.types.f32, dtype=ti.types.f32,
                                        whole_frame=False, **kw))
        assert_close(got, c_oracle.pipeline12_reinhard(packed, work="f32", out="f32", **kw), f"{kind} f32 {kw}")


def test_degenerate_pipeline_full_size(ti, dev):
    from taichi_image_amd.pipeline import pipeline12_reinhard
    for kind in ("zero", "binary"):
        packed = O.encode12(degenerate_cfa(kind, 3072, 4096))
        want = c_oracle.pipeline12_reinhard(packed, out="u8")
        for wf in (True, False):
            got = _host(pipeline12_reinhard(torch.from_numpy(packed).to(dev), dtype=ti.types.u8, whole_frame=wf,
                                            check=True if wf else None))
            assert_close(got, want, f"{kind} whole_frame={wf}")


@pytest.mark.parametrize("din", ["f16", "f32", "u8"])
@pytest.mark.parametrize("kind", DEGENERATE)
def test_degenerate_stateless_tonemaps(ti, kind, din):
    cfa = degenerate_cfa(kind, 24, 40)
    img = O.bayer_to_rgb(O.decode12(O.encode12(cfa), din, scaled=True))
    for gamma in (1.0, 0.5):
        for dout in ("u8", "f16"):
            got = ti.tonemap.tonemap_reinhard(img, gamma=gamma, dtype=getattr(ti.types, dout))
            assert_close(got, O.tonemap_reinhard(img, gamma=gamma, dtype=dout), f"reinhard {kind} {dout} {gamma}")
            got = ti.tonemap.tonemap_linear(img, gamma=gamma, dtype=getattr(ti.types, dout))
            assert_close(got, O.tonemap_linear(img, gamma=gamma, dtype=dout), f"linear {kind} {dout} {gamma}")


@pytest.mark.parametrize("cam", ["Camera16", "Camera32"])
def test_degenerate_frames_in_a_rolling_sequence(ti, dev, cam):
    """Scene, lens cap, blown out, grey card, scene, scene: the state goes through NaN (key = 0/0) and recovers; the
    library's state matches the oracle's at every step."""
    rng = np.random.default_rng(21)
    H, W = 64, 520
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    st = c_oracle.IspState(0.3)
    for step, kind in enumerate(["scene", "zero", "full", "flat", "binary", "scene", "scene"]):
        if kind == "scene":
            frames = [natural_packed12(rng, H, W, dark=0.05 * k) for k in range(2)]
        else:
            frames = [O.encode12(degenerate_cfa(kind, H, W))] * 2
        imgs = [isp.load_packed12(torch.from_numpy(f).to(dev)) for f in frames]
        refs = [_host(im) for im in imgs]
        outs = isp.tonemap_reinhard(imgs, gamma=0.5)
        m = st.update_metering(refs)
        dm = _host(isp.metrics)
        assert_close(dm, m, f"metrics step {step} ({kind})", rel=2e-5)
        for k in range(len(frames)):
            ref_u8, ref_after = c_oracle.reinhard_isp(refs[k], dm, gamma=0.5)
            assert_close(_host(outs[k]), ref_u8, f"u8 step {step} img {k}")
            assert_close(_host(imgs[k]), ref_after, f"p step {step} img {k}", rel=_p_rel(refs[k], dm))
    assert np.isfinite(st.metrics).all(), "the state did not recover"


# ---- C. NaN on the metering subsample ------------------------------------------------------------------------------

def _black_on_grid(rng, H, W):
    """A scene with black 12 x 12 squares centred on stride-8 sample points (the first and the last one among them): after
    a Reinhard call with light_adapt == 1 those samples hold p = 0 / 0 = NaN."""
    r = np.arange(H)[:, None] / H
    c = np.arange(W)[None, :] / W
    v = 0.1 + 0.8 * (0.5 + 0.5 * np.sin(6 * r + 1)) * (0.5 + 0.5 * np.cos(9 * c)) + rng.normal(0, 0.02, (H, W))
    v12 = np.rint(np.clip(v, 0, 1) * 4095).astype(np.uint16)
    lr, lc = (H - 1) // 8 * 8, (W - 1) // 8 * 8
    for (y, x) in [(0, 0), (lr, lc), (H // 16 * 8, W // 16 * 8)]:
        v12[max(0, y - 6):y + 6, max(0, x - 6):x + 6] = 0
    return O.encode12(v12)


@pytest.mark.parametrize("path,cam", [("fused", "Camera16"), ("fused", "Camera32"), ("four_launches", "Camera16"),
                                      ("four_launches", "Camera32"), ("process_packed12", "Camera16")])
def test_nan_on_the_metering_grid(ti, dev, monkeypatch, path, cam):
    """Reinhard with light_adapt == 1 writes p = NaN over black pixels; metering those images again (a supported
    sequence) must follow the rule of the oracle: NaN ignored by min / max, propagated by sums.  (process_packed12 at
    4096 x 3072: the camera-group kernel, f16 only.)"""
    monkeypatch.setenv("MI_ISP_METERING_LAUNCHES", "4" if path == "four_launches" else "1")
    rng = np.random.default_rng(33)
    H, W = (3072, 4096) if path == "process_packed12" else (200, 512)
    frames = [torch.from_numpy(_black_on_grid(rng, H, W)).to(dev) for _ in range(1 if path == "process_packed12" else 2)]
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    st = c_oracle.IspState(0.3)
    if path == "process_packed12":
        outs, imgs = isp.process_packed12(frames, gamma=0.6, keep_images=True)
        refs = [O.isp_load_packed12(_host(f), "f16") for f in frames]
    else:
        imgs = [isp.load_packed12(f) for f in frames]
        refs = [_host(im) for im in imgs]
        outs = isp.tonemap_reinhard(imgs, gamma=0.6)
    m1 = st.update_metering(refs)
    assert_close(_host(isp.metrics), m1, "metrics 1", rel=2e-5)
    for k in range(len(frames)):
        ref_u8, ref_after = c_oracle.reinhard_isp(refs[k], m1, gamma=0.6)
        assert_close(_host(outs[k]), ref_u8, f"u8 1 img {k}")
        assert_close(_host(imgs[k]), ref_after, f"p 1 img {k}")
    mut = [_host(im) for im in imgs]
    assert all(np.isnan(x[::8, ::8]).any() for x in mut), "no NaN on the metering grid"
    outs2 = isp.tonemap_reinhard(imgs, gamma=0.8)
    m2 = st.update_metering(mut)
    assert_close(m2, O.metering_images(mut, 0.7, m1), "the two oracles", rel=2e-5)
    assert np.isfinite(m2[:5]).all() and np.isnan(m2[5]), f"the rule: bounds finite, the mean NaN ({m2})"
    assert_close(_host(isp.metrics), m2, "metrics 2", rel=2e-5)
    for k in range(len(frames)):
        assert_close(_host(outs2[k]), c_oracle.reinhard_isp(mut[k], m2, gamma=0.8)[0], f"u8 2 img {k}")


# ---- D. single-pixel extremes at the decomposition edges -----------------------------------------------------------

def _needle_sites(H, W):
    lr, lc = (H - 1) // 8 * 8, (W - 1) // 8 * 8
    col = (W - 1) // 512 * 512                      # first column of the last (partial) 512-column band
    return {"first": (0, 0),
            "last": (H - 1, W - 1),                 # also the last row of the last 12-row wave band, the last 128 x 32 tile
            "band_last_row": (H // 12 * 12 - 1, W // 2),                   # the last row of the last whole 12-row band
            "tile_first": ((H - 1) // 32 * 32, (W - 1) // 128 * 128),     # the first pixel of the last 128 x 32 tile
            "col_first": (H // 2, col), "col_last": (H // 2, W - 1), "col_before": (H // 2, col - 1),
            "grid_last": (lr, lc), "grid_last_row": (lr, W // 3 // 8 * 8), "grid_last_col": (H // 3 // 8 * 8, lc)}


@pytest.mark.parametrize("needle", ["bright", "dark"])
@pytest.mark.parametrize("shape", [(130, 1544), (36, 520)])
def test_single_pixel_decides(ti, dev, monkeypatch, needle, shape):
    """One CFA pixel at 4095 in a dark frame (or at 0 in a bright one) at the edges of the kernels' decompositions: the
    stateless chains - the whole-frame kernel, the multi-pass chain (f16) and the tile passes (f32 work) - where it decides
    a bound, and the ISP metering + Reinhard, where it decides the subsample bounds (grid sites) or max_out (elsewhere)."""
    from taichi_image_amd.pipeline import pipeline12_reinhard
    H, W = shape
    rng = np.random.default_rng(17)
    base = (rng.random((H, W)) * 400 + 200 if needle == "bright" else rng.random((H, W)) * 400 + 3200).astype(np.uint16)
    val = 4095 if needle == "bright" else 0
    kw = dict(gamma=0.5, light_adapt=0.6)
    base_img = O.isp_load_packed12(O.encode12(base), "f16")
    m0 = c_oracle.IspState(0.3).update_metering([base_img])
    for name, (y, x) in _needle_sites(H, W).items():
        v12 = base.copy()
        v12[y, x] = val
        packed = O.encode12(v12)
        # premise: the needle moves the stateless bounds
        lo0, hi0 = O.bounds(O.bayer_to_rgb(O.decode12(O.encode12(base), "f16", scaled=True)))
        lo1, hi1 = O.bounds(O.bayer_to_rgb(O.decode12(packed, "f16", scaled=True)))
        assert (lo0, hi0) != (lo1, hi1), f"{name}: the needle does not decide a bound"
        want = c_oracle.pipeline12_reinhard(packed, out="f16")
        for wf in (True, False):
            got = _host(pipeline12_reinhard(torch.from_numpy(packed).to(dev), whole_frame=wf, check=True if wf else None))
            assert_close(got, want, f"{name} {(y, x)} whole_frame={wf}")
        got = _host(pipeline12_reinhard(torch.from_numpy(packed).to(dev), work_dtype=ti.types.f32, dtype=ti.types.f32,
                                        whole_frame=False))
        assert_close(got, c_oracle.pipeline12_reinhard(packed, work="f32", out="f32"), f"{name} {(y, x)} f32 multi-pass chain")    # (the stream route: strm::supported takes f32)
        # the ISP: metering on the subsample (a grid needle decides its bounds) and max_out over the whole image
        refs = [O.isp_load_packed12(packed, "f16")]
        m = c_oracle.IspState(0.3).update_metering(refs)
        ref_u8, ref_after = c_oracle.reinhard_isp(refs[0], m, **kw)
        on_grid = name.startswith("grid")
        if on_grid:
            assert not np.array_equal(m[:4], m0[:4]), f"{name}: the needle does not decide the metering bounds"
        else:
            _, p_base = c_oracle.reinhard_isp(base_img, m, **kw)
            assert np.nanmax(ref_after.astype(np.float32)) != np.nanmax(p_base.astype(np.float32)), \
                f"{name}: the needle does not decide max_out"
        for path in ("two_calls", "four_launch_metering", "process"):
            monkeypatch.setenv("MI_ISP_METERING_LAUNCHES", "4" if path == "four_launch_metering" else "1")
            isp = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
            if path == "process":
                outs, imgs = isp.process_packed12([torch.from_numpy(packed).to(dev)], keep_images=True, **kw)
            else:
                imgs = [isp.load_packed12(torch.from_numpy(packed).to(dev))]
                outs = isp.tonemap_reinhard(imgs, **kw)
            assert_close(_host(isp.metrics), m, f"{name} {path} metrics", rel=2e-5)
            assert_close(_host(outs[0]), ref_u8, f"{name} {path} u8")
            assert_close(_host(imgs[0]), ref_after, f"{name} {path} p")


@pytest.mark.parametrize("site", ["last", "grid_last"])
def test_single_pixel_camera_group_full_size(ti, dev, site):
    """4096 x 3072 through the camera-group kernel: a needle at 4095 in a dark frame decides max_out (and, on the grid,
    the metering bounds)."""
    H, W = 3072, 4096
    rng = np.random.default_rng(5)
    base = (rng.random((H, W)) * 400 + 200).astype(np.uint16)
    y, x = _needle_sites(H, W)[site]
    v12 = base.copy()
    v12[y, x] = 4095
    packed = O.encode12(v12)
    refs = [O.isp_load_packed12(packed, "f16")]
    m = c_oracle.IspState(0.3).update_metering(refs)
    _, p_base = c_oracle.reinhard_isp(O.isp_load_packed12(O.encode12(base), "f16"), m, gamma=0.5)
    ref_u8, ref_after = c_oracle.reinhard_isp(refs[0], m, gamma=0.5)
    assert np.nanmax(ref_after.astype(np.float32)) != np.nanmax(p_base.astype(np.float32)), "the needle does not decide max_out"
    isp = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    outs, imgs = isp.process_packed12([torch.from_numpy(packed).to(dev)], gamma=0.5, keep_images=True)
    assert_close(_host(isp.metrics), m, "metrics", rel=2e-5)
    assert_close(_host(outs[0]), ref_u8, "u8")
    assert_close(_host(imgs[0]), ref_after, "p")
