"""Chroma noise reduction (Camera16/32 chroma_denoise=, chroma_denoise, chroma_denoise_yuv420) on the GPU against
tests/chroma_denoise_ref.py, bit for bit.  Through the ISP, the filtering ISP's output must be the restatement applied to the
output of an identical ISP without the operator, with the same metering state and the same mutated images.

The kernel's tile is 64 x 32 cells = 128 x 64 pixels; it takes a dword path when W % 4 == 0 and the image is 4-byte
aligned and a byte path otherwise, and a block whose windows stay inside the cell grid skips the grid test: 134 x 264 has
such a block on the dword path at every radius, 131 x 261 (three tiles each way, odd) on the byte path, and 35 x 132 has
the odd last row on the dword path."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chroma_denoise_ref as C
from tests import local_contrast_ref as R
from tests import sharpen_ref as S
from tests.util import _count_calls, assert_exact, natural_packed12, u8_batch_with_sentinels

pytestmark = pytest.mark.gpu

CAMS = ["Camera16", "Camera32"]
RADII = [1, 2, 3]
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (5, 5), (31, 33), (64, 64), (70, 131), (96, 256), (130, 260), (131, 261), (134, 264), (35, 132)]
YUV_SHAPES = [(2, 2), (4, 6), (30, 34), (64, 96), (66, 100), (130, 260), (134, 264)]
SETTINGS = [(8, 12, 1.0), (255, 255, 1.0), (8, 12, 0.5), (2, 12, 1.0), (8, 3, 1.0), (8, 12, 0.0)]       # (tl, tc, strength)
ENTRY_POINTS = ("mi_isp_chroma_denoise_rgb_batch", "mi_isp_chroma_denoise_yuv420_batch")


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def check_not_vacuous(ref_fn, img, radius, refs, what):
    """The references of the SETTINGS in order: each differs from its input (strength 0 excepted, the identity), from the
    setting before it, and from the two mutants of the restatement (clamped border taps, truncating division)."""
    for k, ref in enumerate(refs):
        tl, tc, strength = SETTINGS[k]
        if k > 0:
            assert not np.array_equal(ref, refs[k - 1]), f"{what}: settings {k - 1} and {k} give the same output"
        if strength > 0:
            assert not np.array_equal(ref, img), f"{what}: setting {k} leaves the input as it is"
            assert not np.array_equal(ref, ref_fn(img, radius, tl, tc, strength, clamp_border=True)), \
                f"{what}: setting {k} does not see clamped border taps"
            assert not np.array_equal(ref, ref_fn(img, radius, tl, tc, strength, truncate=True)), \
                f"{what}: setting {k} does not see a truncating division"


def run_settings(ti, fn, ref_fn, img, t, radius, settings, what):
    refs = []
    for tl, tc, strength in settings:
        ref = ref_fn(img, radius, tl, tc, strength)
        got = fn(t, ti.ChromaDenoise(radius, tl, tc, strength))
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.data_ptr() != t.data_ptr()
        assert_exact(got.cpu().numpy(), ref, f"{what} {(tl, tc, strength)}")
        refs.append(ref)
    assert_exact(t.cpu().numpy(), img, "the input is left alone")
    return refs


# ---- the operator on its own -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", SHAPES)
def test_chroma_denoise_against_the_restatement(ti, rng, dev, radius, H, W):
    scene = S.scene_u8(rng, H, W)
    refs = run_settings(ti, ti.chroma_denoise.chroma_denoise, C.chroma_denoise_rgb, scene, torch.from_numpy(scene).to(dev),
                        radius, SETTINGS, f"scene {H}x{W} R={radius}")
    if H >= 30:
        check_not_vacuous(C.chroma_denoise_rgb, scene, radius, refs, f"scene {H}x{W} R={radius}")
    noise = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)       # (every threshold but 255 leaves random bytes alone)
    ref = run_settings(ti, ti.chroma_denoise.chroma_denoise, C.chroma_denoise_rgb, noise, torch.from_numpy(noise).to(dev),
                       radius, [(255, 255, 1.0)], f"random {H}x{W} R={radius}")[0]
    if H >= 30:
        assert not np.array_equal(ref, noise)
        assert not np.array_equal(ref, C.chroma_denoise_rgb(noise, radius, 255, 255, 1.0, clamp_border=True))
        assert not np.array_equal(ref, C.chroma_denoise_rgb(noise, radius, 255, 255, 1.0, truncate=True))


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", YUV_SHAPES)
def test_chroma_denoise_yuv420_against_the_restatement(ti, rng, dev, radius, H, W):
    scene = C.scene_yuv420(rng, H, W)
    refs = run_settings(ti, ti.chroma_denoise.chroma_denoise_yuv420, C.chroma_denoise_yuv420, scene,
                        torch.from_numpy(scene).to(dev), radius, SETTINGS, f"yuv scene {H}x{W} R={radius}")
    for ref in refs:
        assert_exact(ref[:H], scene[:H], "the Y rows")
    if H >= 30:
        check_not_vacuous(C.chroma_denoise_yuv420, scene, radius, refs, f"yuv scene {H}x{W} R={radius}")
    noise = rng.integers(0, 256, (H * 3 // 2, W)).astype(np.uint8)
    run_settings(ti, ti.chroma_denoise.chroma_denoise_yuv420, C.chroma_denoise_yuv420, noise, torch.from_numpy(noise).to(dev),
                 radius, [(255, 255, 1.0)], f"yuv random {H}x{W} R={radius}")


def test_containers(ti, rng, dev):
    img = S.scene_u8(rng, 31, 33)
    s = ti.ChromaDenoise(2, 8, 12, 0.75)
    ref = C.chroma_denoise_rgb(img, 2, 8, 12, 0.75)
    assert not np.array_equal(ref, img)
    host = ti.chroma_denoise.chroma_denoise(img, s)                   # numpy in, numpy out
    assert isinstance(host, np.ndarray)
    assert_exact(host, ref, "numpy")
    cpu = ti.chroma_denoise.chroma_denoise(torch.from_numpy(img), s)  # torch on the CPU comes back on the CPU
    assert isinstance(cpu, torch.Tensor) and cpu.device.type == "cpu"
    assert_exact(cpu.numpy(), ref, "torch cpu")
    yuv = C.scene_yuv420(rng, 30, 34)
    host = ti.chroma_denoise.chroma_denoise_yuv420(yuv, s)
    assert isinstance(host, np.ndarray)
    assert_exact(host, C.chroma_denoise_yuv420(yuv, 2, 8, 12, 0.75), "numpy yuv")
    with pytest.raises(ValueError):
        ti.chroma_denoise.chroma_denoise(img.astype(np.float32), s)
    with pytest.raises(ValueError):
        ti.chroma_denoise.chroma_denoise(img, (2, 8, 12, 1.0))
    empty = ti.chroma_denoise.chroma_denoise(np.zeros((0, 8, 3), np.uint8), s)
    assert empty.shape == (0, 8, 3)
    assert ti.chroma_denoise.chroma_denoise_yuv420(np.zeros((0, 8), np.uint8), s).shape == (0, 8)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", [(64, 64), (31, 33)])
def test_views_at_odd_byte_offsets_take_the_byte_path(ti, rng, dev, radius, H, W):
    """An image that starts 1, 2 or 3 bytes past a 4-byte boundary (W % 4 == 0 at 64 x 64: only the base is odd)."""
    img = S.scene_u8(rng, H, W)
    ref = C.chroma_denoise_rgb(img, radius, 8, 12, 1.0)
    assert not np.array_equal(ref, img)
    n = H * W * 3
    buf = torch.zeros(n + 8, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        view = buf[off:off + n].view(H, W, 3)
        view.copy_(torch.from_numpy(img))
        assert view.data_ptr() % 4 == (buf.data_ptr() + off) % 4 != 0
        got = ti.chroma_denoise.chroma_denoise(view, ti.ChromaDenoise(radius, 8, 12, 1.0))
        assert_exact(got.cpu().numpy(), ref, f"offset {off}")
    if H % 2 == 0:
        yuv = C.scene_yuv420(rng, H, W)
        ref = C.chroma_denoise_yuv420(yuv, radius, 8, 12, 1.0)
        assert not np.array_equal(ref, yuv)
        for off in (1, 2, 3):
            view = buf[off:off + yuv.size].view(H * 3 // 2, W)
            view.copy_(torch.from_numpy(yuv))
            got = ti.chroma_denoise.chroma_denoise_yuv420(view, ti.ChromaDenoise(radius, 8, 12, 1.0))
            assert_exact(got.cpu().numpy(), ref, f"yuv offset {off}")


@pytest.mark.parametrize("n", [1, 3, 33])
def test_batches(ti, rng, dev, n):
    """33 images cross the 32-per-launch split."""
    H, W = 16, 20
    imgs = [S.scene_u8(rng, H, W, sigma=0.03 + 0.002 * k) for k in range(n)]
    s = ti.ChromaDenoise(2, 8, 12, 1.0)
    outs = ti.chroma_denoise.apply([torch.from_numpy(i).to(dev) for i in imgs], s)
    assert len(outs) == n
    for k in range(n):
        ref = C.chroma_denoise_rgb(imgs[k], 2, 8, 12, 1.0)
        assert not np.array_equal(ref, imgs[k])
        assert_exact(outs[k].cpu().numpy(), ref, f"image {k} of {n}")
    yuvs = [C.scene_yuv420(rng, H, W) for _ in range(n)]
    outs = ti.chroma_denoise.apply([torch.from_numpy(y).to(dev) for y in yuvs], s, yuv420=True)
    for k in range(n):
        ref = C.chroma_denoise_yuv420(yuvs[k], 2, 8, 12, 1.0)
        assert not np.array_equal(ref, yuvs[k])
        assert_exact(outs[k].cpu().numpy(), ref, f"yuv image {k} of {n}")


@pytest.mark.parametrize("H,W", [(8, 16), (6, 10)])
def test_the_second_launch_group(ti, rng, dev, H, W):
    """33 images of distinct contents through the entry points themselves, on the dword path (8 x 16) and on the byte path
    (6 x 10): image 32 is the second group of 32 and, for the planar form, the second copy of the Y rows.  Sentinel bytes
    behind every destination."""
    s, args = ti.ChromaDenoise(2, 8, 12, 1.0), (2, 8, 12, 1.0)
    imgs = [S.scene_u8(rng, H, W, sigma=0.03 + 0.002 * k) for k in range(33)]
    refs = [C.chroma_denoise_rgb(i, *args) for i in imgs]
    assert not np.array_equal(refs[32], imgs[32]) and not np.array_equal(refs[32], refs[0])
    outs = u8_batch_with_sentinels("mi_isp_chroma_denoise_rgb_batch", imgs, H, W, (s._arg(),), dev)
    for k in range(33):
        assert_exact(outs[k], refs[k], f"{H}x{W} image {k}")
    yuvs = [C.scene_yuv420(rng, H, W) for _ in range(33)]
    refs = [C.chroma_denoise_yuv420(y, *args) for y in yuvs]
    assert not np.array_equal(refs[32], yuvs[32])
    outs = u8_batch_with_sentinels("mi_isp_chroma_denoise_yuv420_batch", yuvs, H, W, (s._arg(),), dev)
    for k in range(33):
        assert_exact(outs[k], refs[k], f"{H}x{W} yuv image {k}")


# ---- through the ISP ------------------------------------------------------------------------------------------------------
CDN = dict(radius=2, luma_threshold=8, chroma_threshold=12, strength=1.0)
CDN_ARGS = (2, 8, 12, 1.0)
SHARP = dict(amount=1.5, radius=2, threshold=1, overshoot=10)
SHARP_ARGS = (1.5, 2, 1, 10)
LC = dict(tiles=(2, 3), clip_limit=2.0, strength=0.75)
LC_ARGS = ((2, 3), 2.0, 0.75)
ISP_CASES = ["reinhard", "reinhard_keep", "linear", "only", "process", "process_keep", "rotate_90", "flip_horiz", "resize"]


def isp_pair(ti, dev, cam, on=True, **kw):
    kw = dict(moving_alpha=0.3, device=dev, **kw)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    filt = getattr(ti, cam)(ti.BayerPattern.RGGB, chroma_denoise=ti.ChromaDenoise(**CDN) if on else None, **kw)
    return plain, filt


def run_case(ti, isp, case, frames):
    """(u8 outputs, images left behind or None) of one step of `case` on the packed frames."""
    if case in ("process", "process_keep"):
        if case == "process_keep":
            return isp.process_packed12(frames, gamma=0.7, keep_images=True)
        return isp.process_packed12(frames, gamma=0.7), None
    imgs = isp.load_packed12_batch(frames)
    if case == "linear":
        return isp.tonemap_linear(imgs, gamma=0.8), imgs
    if case == "only":
        isp.update_metering(imgs)
        return [isp.tonemap_only(im, isp.metrics, 0.7, 1.0, 1.0, 0.0) for im in imgs], imgs
    if case == "yuv420":
        return isp.tonemap_reinhard_yuv420(imgs, gamma=0.7), imgs
    return isp.tonemap_reinhard(imgs, gamma=0.7, write_back=case != "reinhard_keep"), imgs


def isp_kwargs(ti, case):
    if case in ("rotate_90", "flip_horiz"):
        return dict(transform=ti.ImageTransform[case])
    return dict(resize_width=48) if case == "resize" else {}


def frames_of(rng, dev, H, W, n):
    return [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(n)]


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("H,W", [(64, 96), (96, 256)])
@pytest.mark.parametrize("case", ISP_CASES)
def test_isp_outputs_are_the_filter_of_the_plain_outputs(ti, rng, dev, monkeypatch, cam, H, W, case):
    frames = frames_of(rng, dev, H, W, 3)
    plain, filt = isp_pair(ti, dev, cam, **isp_kwargs(ti, case))
    group = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard")
    for step in range(2):
        want, want_imgs = run_case(ti, plain, case, frames)
        got, got_imgs = run_case(ti, filt, case, frames)
        what = f"{cam} {case} {H}x{W} step {step}"
        for k, (g, w) in enumerate(zip(got, want)):
            ref = C.chroma_denoise_rgb(w.cpu().numpy(), *CDN_ARGS)
            assert not np.array_equal(ref, w.cpu().numpy()), what
            assert_exact(g.cpu().numpy(), ref, f"{what} output {k}")
        assert_exact(filt.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), what + " metering state")
        if want_imgs is not None:
            for k, (g, w) in enumerate(zip(got_imgs, want_imgs)):
                assert_exact(g.cpu().numpy(), w.cpu().numpy(), f"{what} image {k}")
    if case in ("process", "process_keep"):           # Camera16 takes the one-launch camera group, Camera32 the two calls
        assert len(group) == (4 if cam == "Camera16" else 0), f"{cam}: {len(group)} camera-group launches"


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("H,W,fused", [(64, 96, True), (66, 100, False)])
def test_isp_yuv420_filters_the_chroma_planes(ti, rng, dev, monkeypatch, cam, H, W, fused):
    """W % 16 == 0 takes the fused YUV store, W = 100 the RGB tonemap and the separate conversion: either way the output is
    the planar filter of the plain call's YUV image (not the YUV image of the filtered RGB)."""
    frames = frames_of(rng, dev, H, W, 2)
    plain, filt = isp_pair(ti, dev, cam)
    calls = _count_calls(monkeypatch, "mi_isp_reinhard_batch_yuv420")
    rgb_calls = _count_calls(monkeypatch, "mi_isp_chroma_denoise_rgb_batch")
    for step in range(2):
        want, want_imgs = run_case(ti, plain, "yuv420", frames)
        got, got_imgs = run_case(ti, filt, "yuv420", frames)
        for k, (g, w) in enumerate(zip(got, want)):
            ref = C.chroma_denoise_yuv420(w.cpu().numpy(), *CDN_ARGS)
            assert not np.array_equal(ref, w.cpu().numpy())
            assert_exact(g.cpu().numpy(), ref, f"{cam} yuv420 {H}x{W} step {step} output {k}")
        assert_exact(filt.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), "metering state")
        for g, w in zip(got_imgs, want_imgs):
            assert_exact(g.cpu().numpy(), w.cpu().numpy(), "images")
    assert len(calls) == (4 if fused else 0) and not rgb_calls


@pytest.mark.parametrize("cam", CAMS)
def test_the_order_is_denoise_then_local_contrast_then_sharpen(ti, rng, dev, cam):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 2)
    kw = dict(moving_alpha=0.3, device=dev)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    full = getattr(ti, cam)(ti.BayerPattern.RGGB, chroma_denoise=ti.ChromaDenoise(**CDN), local_contrast=ti.LocalContrast(**LC),
                            sharpen=ti.Sharpen(**SHARP), **kw)
    for case in ("reinhard", "process"):
        want, _ = run_case(ti, plain, case, frames)
        got, _ = run_case(ti, full, case, frames)
        for g, w in zip(got, want):
            w = w.cpu().numpy()
            ref = S.sharpen_rgb(R.clahe_rgb(C.chroma_denoise_rgb(w, *CDN_ARGS), *LC_ARGS), *SHARP_ARGS)
            assert_exact(g.cpu().numpy(), ref, f"{cam} {case}")
            assert not np.array_equal(ref, C.chroma_denoise_rgb(S.sharpen_rgb(R.clahe_rgb(w, *LC_ARGS), *SHARP_ARGS), *CDN_ARGS)), \
                "the order shows"
            assert not np.array_equal(ref, S.sharpen_rgb(R.clahe_rgb(w, *LC_ARGS), *SHARP_ARGS))
    want, _ = run_case(ti, plain, "yuv420", frames)
    got, _ = run_case(ti, full, "yuv420", frames)
    for g, w in zip(got, want):
        w = w.cpu().numpy()
        ref = S.sharpen_yuv420(R.clahe_yuv420(C.chroma_denoise_yuv420(w, *CDN_ARGS), *LC_ARGS), *SHARP_ARGS)
        assert_exact(g.cpu().numpy(), ref, f"{cam} yuv420")


def test_set_turns_it_on_and_off(ti, rng, dev):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 1)
    plain, isp = isp_pair(ti, dev, "Camera32", on=False)
    assert isp.chroma_denoise is None
    s = ti.ChromaDenoise(**CDN)

    def step():
        want = plain.tonemap_reinhard(plain.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()
        return want, isp.tonemap_reinhard(isp.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()

    want, got = step()
    assert_exact(got, want, "off")
    isp.set(chroma_denoise=s)
    assert isp.chroma_denoise == s
    want, got = step()
    assert_exact(got, C.chroma_denoise_rgb(want, *CDN_ARGS), "on with the next call")
    isp.set(moving_alpha=0.3)                                          # (None leaves it)
    assert isp.chroma_denoise == s
    isp.set(chroma_denoise=ti.ChromaDenoise(3, 4, 20, 0.5))
    want, got = step()
    ref = C.chroma_denoise_rgb(want, 3, 4, 20, 0.5)
    assert not np.array_equal(ref, C.chroma_denoise_rgb(want, *CDN_ARGS))
    assert_exact(got, ref, "replaced")
    isp.set(chroma_denoise=False)
    assert isp.chroma_denoise is None
    want, got = step()
    assert_exact(got, want, "off again")
    with pytest.raises(ValueError):
        isp.set(chroma_denoise=1.0)


@pytest.mark.parametrize("cam", CAMS)
def test_without_chroma_denoise_no_new_entry_point_is_called(ti, rng, dev, monkeypatch, cam):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 2)
    counts = [_count_calls(monkeypatch, name) for name in ENTRY_POINTS]
    for case in ISP_CASES + ["yuv420"]:
        isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, sharpen=ti.Sharpen(), local_contrast=ti.LocalContrast((2, 2)),
                               **isp_kwargs(ti, case))
        assert isp.chroma_denoise is None
        run_case(ti, isp, case, frames)
        assert not counts[0] and not counts[1], case
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, chroma_denoise=ti.ChromaDenoise())      # (the probe does count)
    run_case(ti, isp, "reinhard", frames)
    run_case(ti, isp, "yuv420", frames)
    assert len(counts[0]) == 1 and len(counts[1]) == 1


def test_graph_capture_of_a_step(ti, rng, dev):
    """load + tonemap_reinhard with the operator captured once (a single chain of launches) and replayed on new frame
    contents."""
    H, W = 64, 96
    frames = [[torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.02 * ((k + j) % 3))).to(dev)
               for j in range(2)] for k in range(3)]
    static = [torch.empty_like(f) for f in frames[0]]
    cap = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev, chroma_denoise=ti.ChromaDenoise(**CDN))
    eager = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev)

    def step(isp, srcs):
        return isp.tonemap_reinhard(isp.load_packed12_batch(srcs), gamma=0.7, write_back=False)

    for s, f in zip(static, frames[0]):
        s.copy_(f)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step(cap, static)                                    # (warm-up: the first step, eagerly, on the capture stream)
    torch.cuda.current_stream(dev).wait_stream(side)
    step(eager, frames[0])
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        outs = step(cap, static)
    seen = []
    for k in (1, 2):                                         # (a captured update_metering reads the state it was captured with)
        for s, f in zip(static, frames[k]):
            s.copy_(f)
        g.replay()
        probe = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev)
        probe.metrics = eager.metrics.clone()
        want = step(probe, frames[k])
        torch.cuda.synchronize(dev)
        for a, b in zip(outs, want):
            ref = C.chroma_denoise_rgb(b.cpu().numpy(), *CDN_ARGS)
            assert not np.array_equal(ref, b.cpu().numpy())
            assert_exact(a.cpu().numpy(), ref, f"replay {k}")
        seen.append(outs[0].cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]), "the replays saw the same frame"


# ---- C ABI error returns ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_without_a_launch(ti, rng, dev):
    """A bad radius, src == dst and an odd planar size are refused by the host checks: the destination stays as it was."""
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = 8, 12
    img = S.scene_u8(rng, H, W, sigma=0.08)
    src = torch.from_numpy(img).to(dev)
    dst = torch.full((H, W, 3), 99, dtype=torch.uint8, device=dev)
    good = _native.ChromaDenoise(1, 255, 255, 64)
    stream = _native.stream_ptr(dev)
    for fn, h in ((L.mi_isp_chroma_denoise_rgb_batch, H), (L.mi_isp_chroma_denoise_yuv420_batch, 16)):
        for args in ((_native.ptr_array([src]), _native.ptr_array([dst]), 1, h, W, _native.ChromaDenoise(4, 8, 12, 64), stream),
                     (_native.ptr_array([src]), _native.ptr_array([dst]), 1, h, W, _native.ChromaDenoise(1, 8, 12, 65), stream),
                     (_native.ptr_array([src]), _native.ptr_array([src]), 1, h, W, good, stream),
                     (_native.ptr_array([src]), _native.ptr_array([dst]), -1, h, W, good, stream)):
            assert fn(*args) == 1
            assert b"chroma_denoise" in L.mi_isp_last_error()
    assert L.mi_isp_chroma_denoise_yuv420_batch(_native.ptr_array([src]), _native.ptr_array([dst]), 1, 15, W, good, stream) == 1
    assert L.mi_isp_chroma_denoise_rgb_batch(_native.ptr_array([src]), _native.ptr_array([dst]), 0, H, W, good, stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((dst == 99).all())
    assert_exact(src.cpu().numpy(), img, "the source")
    assert L.mi_isp_chroma_denoise_rgb_batch(_native.ptr_array([src]), _native.ptr_array([dst]), 1, H, W, good, stream) == 0
    ref = C.chroma_denoise_rgb(img, 1, 255, 255, 1.0)
    assert not np.array_equal(ref, img)
    assert_exact(dst.cpu().numpy(), ref, "the good call")
