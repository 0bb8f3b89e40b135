"""Luma noise reduction (Camera16/32 luma_denoise=, luma_denoise, luma_denoise_yuv420) on the GPU against
tests/luma_denoise_ref.py, bit for bit.  Through the ISP, the filtering ISP's output must be the restatement applied to the
output of an identical ISP without the operator, with the same metering state and the same mutated images.

The kernel's tile is 128 x 64 pixels, a thread owns 4 columns by 8 rows, and the staged lumas reach 4 columns and r rows
past the tile.  It takes a dword path when W % 4 == 0 and the image is 4-byte aligned and a byte path otherwise, and a
block whose windows stay inside the image skips the inside test.  Why each shape is here:
  (1, 1)      one pixel: every tap but the centre is outside the image
  (1, 9)      one row on the byte path: no tap above or below; three 4-column groups, the last with one pixel
  (9, 1)      one column: no tap left or right; two 8-row strips, the second with one row
  (2, 3)      smaller than every window: the image bounds all four sides of every window at once
  (5, 5)      the 5 x 5 window of the centre pixel is the image; at radius 3 every window is cut
  (31, 33)    odd sides on the byte path, a last group of one pixel and a last strip of seven rows
  (64, 64)    one tile's height, half its width, on the dword path: every block row and column is a border
  (134, 264)  3 x 3 blocks on the dword path; the middle block skips the inside test at every radius; the last block row
              has 6 rows, the last block column 8 columns
  (131, 261)  3 x 3 blocks, odd sides, on the byte path (the middle block skips the inside test there too)
  (35, 132)   a short last row band (3 rows in the fifth strip) and a second block column of one group on the dword path
The planar shapes are even: (2, 2) and (4, 6) below every window, (30, 34) and (130, 262) on the byte path (W % 4 == 2; the
latter 3 x 3 blocks), (64, 64), (134, 264) and (36, 132) on the dword path as above.
The scenes are those of tests/test_luma_denoise_cpu.py (the same seeds), which shows that on them every setting's reference
differs from its input, from its neighbour and from each mutant of the restatement."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chroma_denoise_ref as C
from tests import color_lut_ref as CL
from tests import local_contrast_ref as R
from tests import luma_denoise_ref as Y
from tests import sharpen_ref as S
from tests.util import _count_calls, assert_exact, natural_packed12, u8_batch_with_sentinels

pytestmark = pytest.mark.gpu

CAMS = ["Camera16", "Camera32"]
RADII = [1, 2, 3]
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (5, 5), (31, 33), (64, 64), (134, 264), (131, 261), (35, 132)]
YUV_SHAPES = [(2, 2), (4, 6), (30, 34), (64, 64), (134, 264), (36, 132), (130, 262)]
SETTINGS = [(6, 14, 1.0), (255, 255, 1.0), (6, 14, 0.5), (2, 14, 1.0), (6, 3, 1.0), (6, 14, 0.0)]          # (t0, t1, strength)
ENTRY_POINTS = ("mi_isp_luma_denoise_rgb_batch", "mi_isp_luma_denoise_yuv420_batch")


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def run_settings(ti, fn, ref_fn, img, t, radius, settings, what):
    refs = []
    for t0, t1, strength in settings:
        ref = ref_fn(img, radius, t0, t1, strength)
        got = fn(t, ti.LumaDenoise(radius, t0, t1, strength))
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.data_ptr() != t.data_ptr()
        assert_exact(got.cpu().numpy(), ref, f"{what} {(t0, t1, strength)}")
        refs.append(ref)
    assert_exact(t.cpu().numpy(), img, "the input is left alone")
    return refs


# ---- the operator on its own -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", SHAPES)
def test_luma_denoise_against_the_restatement(ti, dev, radius, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    scene = S.scene_u8(rng, H, W)
    refs = run_settings(ti, ti.luma_denoise.luma_denoise, Y.luma_denoise_rgb, scene, torch.from_numpy(scene).to(dev), radius,
                        SETTINGS, f"scene {H}x{W} R={radius}")
    if H >= 30:
        assert not np.array_equal(refs[0], scene) and not np.array_equal(refs[0], refs[1])
    noise = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)        # (random bytes: threshold 255 is the mean of the taps)
    ref = run_settings(ti, ti.luma_denoise.luma_denoise, Y.luma_denoise_rgb, noise, torch.from_numpy(noise).to(dev), radius,
                       [(255, 255, 1.0), (40, 90, 1.0)], f"random {H}x{W} R={radius}")[0]
    if H >= 30:
        assert not np.array_equal(ref, noise)
        assert not np.array_equal(ref, Y.luma_denoise_rgb(noise, radius, 255, 255, 1.0, clamp_border=True))


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", YUV_SHAPES)
def test_luma_denoise_yuv420_against_the_restatement(ti, dev, radius, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    scene = C.scene_yuv420(rng, H, W)
    refs = run_settings(ti, ti.luma_denoise.luma_denoise_yuv420, Y.luma_denoise_yuv420, scene,
                        torch.from_numpy(scene).to(dev), radius, SETTINGS, f"yuv scene {H}x{W} R={radius}")
    for ref in refs:
        assert_exact(ref[H:], scene[H:], "the chroma rows")
    if H >= 30:
        assert not np.array_equal(refs[0], scene) and not np.array_equal(refs[0], refs[1])
    noise = rng.integers(0, 256, (H * 3 // 2, W)).astype(np.uint8)
    ref = run_settings(ti, ti.luma_denoise.luma_denoise_yuv420, Y.luma_denoise_yuv420, noise, torch.from_numpy(noise).to(dev),
                       radius, [(255, 255, 1.0)], f"yuv random {H}x{W} R={radius}")[0]
    assert_exact(ref[H:], noise[H:], "the chroma rows of random bytes")


def test_containers(ti, dev):
    rng = np.random.default_rng(31033)
    img = S.scene_u8(rng, 31, 33)
    s = ti.LumaDenoise(2, 6, 14, 0.75)
    ref = Y.luma_denoise_rgb(img, 2, 6, 14, 0.75)
    assert not np.array_equal(ref, img)
    host = ti.luma_denoise.luma_denoise(img, s)                       # numpy in, numpy out
    assert isinstance(host, np.ndarray)
    assert_exact(host, ref, "numpy")
    cpu = ti.luma_denoise.luma_denoise(torch.from_numpy(img), s)      # torch on the CPU comes back on the CPU
    assert isinstance(cpu, torch.Tensor) and cpu.device.type == "cpu"
    assert_exact(cpu.numpy(), ref, "torch cpu")
    assert_exact(ti.luma_denoise.luma_denoise(img, ti.LumaDenoise(2, 6, None, 1.0)), Y.luma_denoise_rgb(img, 2, 6, 6, 1.0),
                 "threshold_bright=None is threshold")
    yuv = C.scene_yuv420(rng, 30, 34)
    host = ti.luma_denoise.luma_denoise_yuv420(yuv, s)
    assert isinstance(host, np.ndarray)
    assert_exact(host, Y.luma_denoise_yuv420(yuv, 2, 6, 14, 0.75), "numpy yuv")
    with pytest.raises(ValueError):
        ti.luma_denoise.luma_denoise(img.astype(np.float32), s)
    with pytest.raises(ValueError):
        ti.luma_denoise.luma_denoise(img, (2, 6, 14, 1.0))
    empty = ti.luma_denoise.luma_denoise(np.zeros((0, 8, 3), np.uint8), s)
    assert empty.shape == (0, 8, 3)
    assert ti.luma_denoise.luma_denoise_yuv420(np.zeros((0, 8), np.uint8), s).shape == (0, 8)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("H,W", [(64, 64), (31, 33)])
def test_views_at_odd_byte_offsets_take_the_byte_path(ti, dev, radius, H, W):
    """An image that starts 1, 2 or 3 bytes past a 4-byte boundary (W % 4 == 0 at 64 x 64: only the base is odd)."""
    rng = np.random.default_rng(H * 1000 + W)
    img = S.scene_u8(rng, H, W)
    ref = Y.luma_denoise_rgb(img, radius, 6, 14, 1.0)
    assert not np.array_equal(ref, img)
    n = H * W * 3
    buf = torch.zeros(n + 8, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        view = buf[off:off + n].view(H, W, 3)
        view.copy_(torch.from_numpy(img))
        assert view.data_ptr() % 4 == (buf.data_ptr() + off) % 4 != 0
        got = ti.luma_denoise.luma_denoise(view, ti.LumaDenoise(radius, 6, 14, 1.0))
        assert_exact(got.cpu().numpy(), ref, f"offset {off}")
    if H % 2 == 0:
        yuv = C.scene_yuv420(rng, H, W)
        ref = Y.luma_denoise_yuv420(yuv, radius, 6, 14, 1.0)
        assert not np.array_equal(ref, yuv)
        for off in (1, 2, 3):
            view = buf[off:off + yuv.size].view(H * 3 // 2, W)
            view.copy_(torch.from_numpy(yuv))
            got = ti.luma_denoise.luma_denoise_yuv420(view, ti.LumaDenoise(radius, 6, 14, 1.0))
            assert_exact(got.cpu().numpy(), ref, f"yuv offset {off}")


@pytest.mark.parametrize("n", [1, 3, 33])
def test_batches(ti, rng, dev, n):
    """33 images cross the 32-per-launch split."""
    H, W = 16, 20
    imgs = [S.scene_u8(rng, H, W, sigma=0.03 + 0.002 * k) for k in range(n)]
    s = ti.LumaDenoise(2, 6, 14, 1.0)
    outs = ti.luma_denoise.apply([torch.from_numpy(i).to(dev) for i in imgs], s)
    assert len(outs) == n
    for k in range(n):
        ref = Y.luma_denoise_rgb(imgs[k], 2, 6, 14, 1.0)
        assert not np.array_equal(ref, imgs[k])
        assert_exact(outs[k].cpu().numpy(), ref, f"image {k} of {n}")
    yuvs = [C.scene_yuv420(rng, H, W) for _ in range(n)]
    outs = ti.luma_denoise.apply([torch.from_numpy(y).to(dev) for y in yuvs], s, yuv420=True)
    for k in range(n):
        ref = Y.luma_denoise_yuv420(yuvs[k], 2, 6, 14, 1.0)
        assert not np.array_equal(ref, yuvs[k])
        assert_exact(outs[k].cpu().numpy(), ref, f"yuv image {k} of {n}")


@pytest.mark.parametrize("H,W", [(8, 16), (6, 10)])
def test_the_second_launch_group(ti, rng, dev, H, W):
    """33 images of distinct contents through the entry points themselves, on the dword path (8 x 16) and on the byte path
    (6 x 10): image 32 is the second group of 32 and, for the planar form, the second copy of the chroma rows.  Sentinel bytes
    behind every destination."""
    s, args = ti.LumaDenoise(2, 6, 14, 1.0), (2, 6, 14, 1.0)
    imgs = [S.scene_u8(rng, H, W, sigma=0.03 + 0.002 * k) for k in range(33)]
    refs = [Y.luma_denoise_rgb(i, *args) for i in imgs]
    assert not np.array_equal(refs[32], imgs[32]) and not np.array_equal(refs[32], refs[0])
    outs = u8_batch_with_sentinels("mi_isp_luma_denoise_rgb_batch", imgs, H, W, (s._arg(),), dev)
    for k in range(33):
        assert_exact(outs[k], refs[k], f"{H}x{W} image {k}")
    yuvs = [C.scene_yuv420(rng, H, W) for _ in range(33)]
    refs = [Y.luma_denoise_yuv420(y, *args) for y in yuvs]
    assert not np.array_equal(refs[32], yuvs[32])
    outs = u8_batch_with_sentinels("mi_isp_luma_denoise_yuv420_batch", yuvs, H, W, (s._arg(),), dev)
    for k in range(33):
        assert_exact(outs[k], refs[k], f"{H}x{W} yuv image {k}")


# ---- through the ISP ------------------------------------------------------------------------------------------------------
LDN = dict(radius=2, threshold=6, threshold_bright=14, strength=1.0)
LDN_ARGS = (2, 6, 14, 1.0)
CDN_ARGS = (2, 8, 12, 1.0)
SHARP_ARGS = (1.5, 2, 1, 10)
LC_ARGS = ((2, 3), 2.0, 0.75)
LUT_N, LUT_STRENGTH = 17, 0.75
ISP_CASES = ["reinhard", "linear", "process", "process_keep", "rotate_90"]


def isp_pair(ti, dev, cam, on=True, **kw):
    kw = dict(moving_alpha=0.3, device=dev, **kw)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    filt = getattr(ti, cam)(ti.BayerPattern.RGGB, luma_denoise=ti.LumaDenoise(**LDN) if on else None, **kw)
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
    if case == "yuv420":
        return isp.tonemap_reinhard_yuv420(imgs, gamma=0.7), imgs
    return isp.tonemap_reinhard(imgs, gamma=0.7), imgs


def isp_kwargs(ti, case):
    return dict(transform=ti.ImageTransform[case]) if case == "rotate_90" else {}


def frames_of(rng, dev, H, W, n):
    return [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(n)]


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("H,W", [(64, 96), (96, 256)])
@pytest.mark.parametrize("case", ISP_CASES)
def test_isp_outputs_are_the_filter_of_the_plain_outputs(ti, rng, dev, cam, H, W, case):
    frames = frames_of(rng, dev, H, W, 2)
    plain, filt = isp_pair(ti, dev, cam, **isp_kwargs(ti, case))
    for step in range(2):
        want, want_imgs = run_case(ti, plain, case, frames)
        got, got_imgs = run_case(ti, filt, case, frames)
        what = f"{cam} {case} {H}x{W} step {step}"
        for k, (g, w) in enumerate(zip(got, want)):
            ref = Y.luma_denoise_rgb(w.cpu().numpy(), *LDN_ARGS)
            assert not np.array_equal(ref, w.cpu().numpy()), what
            assert_exact(g.cpu().numpy(), ref, f"{what} output {k}")
        assert_exact(filt.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), what + " metering state")
        if want_imgs is not None:
            for k, (g, w) in enumerate(zip(got_imgs, want_imgs)):
                assert_exact(g.cpu().numpy(), w.cpu().numpy(), f"{what} image {k}")


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("H,W,fused", [(64, 96, True), (96, 256, True), (66, 100, False)])
def test_isp_yuv420_filters_the_y_plane(ti, rng, dev, monkeypatch, cam, H, W, fused):
    """W % 16 == 0 takes the fused YUV store, W = 100 the RGB tonemap and the separate conversion: either way the output is
    the planar filter of the plain call's YUV image (not the YUV image of the filtered RGB)."""
    frames = frames_of(rng, dev, H, W, 2)
    plain, filt = isp_pair(ti, dev, cam)
    calls = _count_calls(monkeypatch, "mi_isp_reinhard_batch_yuv420")
    rgb_calls = _count_calls(monkeypatch, "mi_isp_luma_denoise_rgb_batch")
    for step in range(2):
        want, want_imgs = run_case(ti, plain, "yuv420", frames)
        got, got_imgs = run_case(ti, filt, "yuv420", frames)
        for k, (g, w) in enumerate(zip(got, want)):
            ref = Y.luma_denoise_yuv420(w.cpu().numpy(), *LDN_ARGS)
            assert not np.array_equal(ref, w.cpu().numpy())
            assert_exact(ref[H:], w.cpu().numpy()[H:], "the chroma rows")
            assert_exact(g.cpu().numpy(), ref, f"{cam} yuv420 {H}x{W} step {step} output {k}")
        assert_exact(filt.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), "metering state")
        for g, w in zip(got_imgs, want_imgs):
            assert_exact(g.cpu().numpy(), w.cpu().numpy(), "images")
    assert len(calls) == (4 if fused else 0) and not rgb_calls


@pytest.mark.parametrize("cam", CAMS)
def test_the_order_is_lut_chroma_luma_local_contrast_sharpen(ti, rng, dev, cam):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 2)
    kw = dict(moving_alpha=0.3, device=dev)
    table = CL.gpu_tables(LUT_N)["look"]
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    full = getattr(ti, cam)(ti.BayerPattern.RGGB, color_lut=ti.ColorLut(table, LUT_STRENGTH),
                            chroma_denoise=ti.ChromaDenoise(*CDN_ARGS), luma_denoise=ti.LumaDenoise(**LDN),
                            local_contrast=ti.LocalContrast(*LC_ARGS), sharpen=ti.Sharpen(*SHARP_ARGS), **kw)

    def tail(x):
        return S.sharpen_rgb(R.clahe_rgb(x, *LC_ARGS), *SHARP_ARGS)

    for case in ("reinhard", "process"):
        want, _ = run_case(ti, plain, case, frames)
        got, _ = run_case(ti, full, case, frames)
        for g, w in zip(got, want):
            head = C.chroma_denoise_rgb(CL.color_lut_rgb(w.cpu().numpy(), table, LUT_STRENGTH), *CDN_ARGS)
            ref = tail(Y.luma_denoise_rgb(head, *LDN_ARGS))
            assert_exact(g.cpu().numpy(), ref, f"{cam} {case}")
            # the order shows: the luma filter before the chroma filter, behind local contrast, behind sharpening, or absent
            lut = CL.color_lut_rgb(w.cpu().numpy(), table, LUT_STRENGTH)
            assert not np.array_equal(ref, tail(C.chroma_denoise_rgb(Y.luma_denoise_rgb(lut, *LDN_ARGS), *CDN_ARGS)))
            assert not np.array_equal(ref, S.sharpen_rgb(Y.luma_denoise_rgb(R.clahe_rgb(head, *LC_ARGS), *LDN_ARGS), *SHARP_ARGS))
            assert not np.array_equal(ref, Y.luma_denoise_rgb(tail(head), *LDN_ARGS))
            assert not np.array_equal(ref, tail(head))
    planar = getattr(ti, cam)(ti.BayerPattern.RGGB, chroma_denoise=ti.ChromaDenoise(*CDN_ARGS), luma_denoise=ti.LumaDenoise(**LDN),
                              local_contrast=ti.LocalContrast(*LC_ARGS), sharpen=ti.Sharpen(*SHARP_ARGS), **kw)
    want, _ = run_case(ti, plain, "yuv420", frames)
    got, _ = run_case(ti, planar, "yuv420", frames)
    for g, w in zip(got, want):
        head = Y.luma_denoise_yuv420(C.chroma_denoise_yuv420(w.cpu().numpy(), *CDN_ARGS), *LDN_ARGS)
        assert_exact(g.cpu().numpy(), S.sharpen_yuv420(R.clahe_yuv420(head, *LC_ARGS), *SHARP_ARGS), f"{cam} yuv420")


def test_set_turns_it_on_and_off(ti, rng, dev):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 1)
    plain, isp = isp_pair(ti, dev, "Camera32", on=False)
    assert isp.luma_denoise is None
    s = ti.LumaDenoise(**LDN)

    def step():
        want = plain.tonemap_reinhard(plain.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()
        return want, isp.tonemap_reinhard(isp.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()

    want, got = step()
    assert_exact(got, want, "off")
    isp.set(luma_denoise=s)
    assert isp.luma_denoise == s
    want, got = step()
    assert_exact(got, Y.luma_denoise_rgb(want, *LDN_ARGS), "on with the next call")
    isp.set(moving_alpha=0.3)                                          # (None leaves it)
    assert isp.luma_denoise == s
    isp.set(luma_denoise=ti.LumaDenoise(3, 4, 20, 0.5))
    want, got = step()
    ref = Y.luma_denoise_rgb(want, 3, 4, 20, 0.5)
    assert not np.array_equal(ref, Y.luma_denoise_rgb(want, *LDN_ARGS))
    assert_exact(got, ref, "replaced")
    isp.set(luma_denoise=False)
    assert isp.luma_denoise is None
    want, got = step()
    assert_exact(got, want, "off again")
    with pytest.raises(ValueError):
        isp.set(luma_denoise=1.0)


@pytest.mark.parametrize("cam", CAMS)
def test_without_luma_denoise_no_new_entry_point_is_called(ti, rng, dev, monkeypatch, cam):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 2)
    counts = [_count_calls(monkeypatch, name) for name in ENTRY_POINTS]
    for case in ISP_CASES + ["yuv420"]:
        isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, sharpen=ti.Sharpen(), local_contrast=ti.LocalContrast((2, 2)),
                               chroma_denoise=ti.ChromaDenoise(), **isp_kwargs(ti, case))
        assert isp.luma_denoise is None
        run_case(ti, isp, case, frames)
        assert not counts[0] and not counts[1], case
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, luma_denoise=ti.LumaDenoise())          # (the probe does count)
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
    cap = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev, luma_denoise=ti.LumaDenoise(**LDN))
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
            ref = Y.luma_denoise_rgb(b.cpu().numpy(), *LDN_ARGS)
            assert not np.array_equal(ref, b.cpu().numpy())
            assert_exact(a.cpu().numpy(), ref, f"replay {k}")
        seen.append(outs[0].cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]), "the replays saw the same frame"


# ---- C ABI error returns ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_without_a_launch(ti, rng, dev):
    """A bad radius, src == dst, overlapping images and an odd planar size are refused by the host checks: the destination
    stays as it was."""
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = 8, 12
    img = S.scene_u8(rng, H, W, sigma=0.08)
    src = torch.from_numpy(img).to(dev)
    dst = torch.full((H, W, 3), 99, dtype=torch.uint8, device=dev)
    good = _native.LumaDenoise(1, 255, 255, 64)
    stream = _native.stream_ptr(dev)
    for fn, h in ((L.mi_isp_luma_denoise_rgb_batch, H), (L.mi_isp_luma_denoise_yuv420_batch, 16)):
        for args in ((_native.ptr_array([src]), _native.ptr_array([dst]), 1, h, W, _native.LumaDenoise(4, 6, 14, 64), stream),
                     (_native.ptr_array([src]), _native.ptr_array([dst]), 1, h, W, _native.LumaDenoise(1, 6, 14, 65), stream),
                     (_native.ptr_array([src]), _native.ptr_array([src]), 1, h, W, good, stream),
                     (_native.ptr_array([src]), _native.ptr_array([src.view(-1)[W:]]), 1, h // 2, W, good, stream),
                     (_native.ptr_array([src]), _native.ptr_array([dst]), -1, h, W, good, stream)):
            assert fn(*args) == 1
            assert b"luma_denoise" in L.mi_isp_last_error()
    assert L.mi_isp_luma_denoise_yuv420_batch(_native.ptr_array([src]), _native.ptr_array([dst]), 1, 15, W, good, stream) == 1
    assert L.mi_isp_luma_denoise_rgb_batch(_native.ptr_array([src]), _native.ptr_array([dst]), 0, H, W, good, stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((dst == 99).all())
    assert_exact(src.cpu().numpy(), img, "the source")
    assert L.mi_isp_luma_denoise_rgb_batch(_native.ptr_array([src]), _native.ptr_array([dst]), 1, H, W, good, stream) == 0
    ref = Y.luma_denoise_rgb(img, 1, 255, 255, 1.0)
    assert not np.array_equal(ref, img)
    assert_exact(dst.cpu().numpy(), ref, "the good call")
