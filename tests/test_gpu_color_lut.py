"""The 3D colour LUT (Camera16/32 color_lut=, color_lut.apply_lut, the C entry points) on the GPU against
tests/color_lut_ref.py, bit for bit.  Through the ISP, the output of the ISP with a LUT must be the restatement applied to the
output of an identical ISP without it, with the same metering state and the same mutated images.

The kernel has three instances: the table in LDS for N <= 17 and for N <= 33, and in global memory (N up to 65, or where the
dispatcher prefers it); mi_isp_color_lut_rgb_batch_path runs a given one.  It takes a dword path when W * 3 % 4 == 0 and the
images are 4-byte aligned and a byte path otherwise; a thread owns 4 pixels, so (1, 1), (1, 5) and (3, 7) end in a partial
thread on the byte path and (5, 4) is the smallest dword image.  The tables, images and shapes come from
tests/color_lut_ref.py, where tests/test_color_lut_cpu.py shows that they are not vacuous."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chroma_denoise_ref as CD
from tests import color_lut_ref as C
from tests import local_contrast_ref as R
from tests import sharpen_ref as S
from tests.util import _count_calls, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = ["Camera16", "Camera32"]
ENTRY_POINTS = ("mi_isp_color_lut_rgb_batch", "mi_isp_color_lut_rgb_batch_path")
AUTO, LDS, GLOBAL = 0, 1, 2
LDS_CHUNK = 4096                  # pixels per trip of an LDS block's chunk loop (csrc/isp_color_lut.h: LDS_CHUNK)
LDS_MAX_POINTS = 33


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def paths_of(N):
    return (LDS, GLOBAL) if N <= LDS_MAX_POINTS else (GLOBAL,)


def abi(ti, srcs, dsts, H, W, lut, path=None):
    """The entry point (path None) or its _path twin on device tensors; the status."""
    from taichi_image_amd import _native
    L = _native.lib()
    dev = srcs[0].device
    table = lut._device_table(dev)
    args = (_native.ptr_array(srcs), _native.ptr_array(dsts), len(srcs), H, W, table.data_ptr(), lut._arg())
    if path is None:
        return L.mi_isp_color_lut_rgb_batch(*args, _native.stream_ptr(dev))
    return L.mi_isp_color_lut_rgb_batch_path(*args, path, _native.stream_ptr(dev))


# ---- the operator on its own -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.GPU_POINTS)
@pytest.mark.parametrize("H,W", C.GPU_SHAPES)
def test_color_lut_against_the_restatement(ti, dev, N, H, W):
    for iname, img in C.gpu_images(H, W).items():
        if iname == "ties" and (H, W) != C.GPU_SHAPES[0] and (H, W) != C.GPU_SHAPES[-1]:
            continue                                              # (its own shape: twice per N is enough)
        h, w = img.shape[:2]
        t = torch.from_numpy(img).to(dev)
        for tname, table in C.gpu_tables(N).items():
            for strength in C.GPU_STRENGTHS:
                what = f"N={N} {tname} table, {iname} image {h}x{w}, strength {strength}"
                ref = C.color_lut_rgb(img, table, strength)
                if tname == "identity" or strength == 0.0:
                    assert_exact(ref, img, what + ": the identity")
                lut = ti.ColorLut(table, strength)
                got = ti.color_lut.apply_lut(t, lut)              # (the dispatcher's path)
                assert isinstance(got, torch.Tensor) and got.device == t.device and got.data_ptr() != t.data_ptr()
                assert_exact(got.cpu().numpy(), ref, what)
                for path in paths_of(N):
                    dst = torch.empty_like(t)
                    assert abi(ti, [t], [dst], h, w, lut, path) == 0
                    assert_exact(dst.cpu().numpy(), ref, f"{what}, path {path}")
        assert_exact(t.cpu().numpy(), img, "the input is left alone")


# ---- through the C ABI -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 33, 65])
def test_views_at_odd_byte_offsets_take_the_byte_path(ti, dev, N):
    """A dword-shaped image (64 x 64) whose source, destination or both start 1, 2 or 3 bytes past a 4-byte boundary."""
    H, W = 64, 64
    img = C.gpu_images(H, W)["scene"]
    lut = ti.ColorLut(C.gpu_tables(N)["look"], 1.0)
    ref = C.color_lut_rgb(img, lut.table)
    n = H * W * 3
    a, b = torch.zeros(n + 8, dtype=torch.uint8, device=dev), torch.zeros(n + 8, dtype=torch.uint8, device=dev)
    for so, do in ((1, 0), (0, 3), (2, 2), (3, 1)):
        src, dst = a[so:so + n].view(H, W, 3), b[do:do + n].view(H, W, 3)
        src.copy_(torch.from_numpy(img))
        b.fill_(7)
        assert src.data_ptr() % 4 == (a.data_ptr() + so) % 4 and dst.data_ptr() % 4 == (b.data_ptr() + do) % 4
        for path in paths_of(N):
            assert abi(ti, [src], [dst], H, W, lut, path) == 0
            assert_exact(dst.cpu().numpy(), ref, f"N={N} offsets {so}, {do} path {path}")
        assert bool((b[:do] == 7).all()) and bool((b[do + n:] == 7).all()), "bytes around the destination"
        assert_exact(src.cpu().numpy(), img, "the source")


@pytest.mark.parametrize("N", [3, 33, 34])
@pytest.mark.parametrize("H,W", [(31, 33), (64, 64)])
def test_in_place_and_out_of_place(ti, dev, N, H, W):
    img = C.gpu_images(H, W)["random"]
    lut = ti.ColorLut(C.gpu_tables(N)["random"], 1.0)
    ref = C.color_lut_rgb(img, lut.table)
    for path in (None,) + paths_of(N):
        src = torch.from_numpy(img).to(dev)
        dst = torch.empty_like(src)
        assert abi(ti, [src], [dst], H, W, lut, path) == 0
        assert_exact(dst.cpu().numpy(), ref, f"out of place, path {path}")
        assert_exact(src.cpu().numpy(), img, "the input is untouched")
        assert abi(ti, [src], [src], H, W, lut, path) == 0         # src == dst
        assert_exact(src.cpu().numpy(), ref, f"in place, path {path}")
    outs = ti.color_lut.apply([torch.from_numpy(img).to(dev)], lut, inplace=True)
    assert_exact(outs[0].cpu().numpy(), ref, "apply(inplace=True)")


@pytest.mark.parametrize("n", [1, 6, 33])
def test_batches(ti, rng, dev, n):
    """33 images cross the 32-per-launch split."""
    H, W = 31, 33
    imgs = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]
    for N in (17, 33, 34):
        lut = ti.ColorLut(C.gpu_tables(N)["random"], 0.5)
        refs = [C.color_lut_rgb(im, lut.table, 0.5) for im in imgs]
        for path in (None,) + paths_of(N):
            srcs = [torch.from_numpy(im).to(dev) for im in imgs]
            dsts = [torch.zeros_like(s) for s in srcs]
            assert abi(ti, srcs, dsts, H, W, lut, path) == 0
            for k in range(n):
                assert_exact(dsts[k].cpu().numpy(), refs[k], f"N={N} image {k} of {n}, path {path}")
        outs = ti.color_lut.apply([torch.from_numpy(im).to(dev) for im in imgs], lut)
        assert len(outs) == n
        for k in range(n):
            assert_exact(outs[k].cpu().numpy(), refs[k], f"N={N} apply image {k} of {n}")


def test_every_block_makes_two_trips_through_its_chunk_loop(ti, rng, dev):
    """The N = 33 instance launches at most one block per CU, and a block takes chunks of LDS_CHUNK consecutive pixels, block
    b the chunks b, b + blocks, ...: two images of (CUs + 1) x LDS_CHUNK pixels are 2 CUs + 2 chunks, so every block makes
    at least two trips and two of them three.  Both images hold the same bytes: one reference."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    H, W = cus + 1, LDS_CHUNK
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    for N, tname in ((33, "random"), (17, "look")):
        lut = ti.ColorLut(C.gpu_tables(N)[tname], 1.0)
        ref = C.color_lut_rgb(img, lut.table)
        assert not np.array_equal(ref, img)
        for path in (LDS, None):
            srcs = [torch.from_numpy(img).to(dev) for _ in range(2)]
            dsts = [torch.zeros_like(s) for s in srcs]
            assert abi(ti, srcs, dsts, H, W, lut, path) == 0
            for k in range(2):
                assert_exact(dsts[k].cpu().numpy(), ref, f"N={N} image {k}, path {path}")


def test_entry_points_refuse_without_a_launch(ti, dev):
    """Every rejected argument gives a non-zero status and a message naming "color_lut", and the destination stays as it
    was; the no-ops succeed."""
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = 8, 12
    img = C.gpu_images(31, 33)["random"][:H, :W].copy()
    src = torch.from_numpy(img).to(dev)
    dst = torch.full((H, W, 3), 99, dtype=torch.uint8, device=dev)
    lut = ti.ColorLut(C.gpu_tables(17)["random"])
    table = lut._device_table(dev).data_ptr()
    good = lut._arg()
    stream = _native.stream_ptr(dev)
    ps, pd = _native.ptr_array([src]), _native.ptr_array([dst])
    null = (type(ps))(None)
    for args in ((ps, pd, 1, H, W, table, _native.ColorLut(1, 64)), (ps, pd, 1, H, W, table, _native.ColorLut(66, 64)),
                 (ps, pd, 1, H, W, table, _native.ColorLut(17, 65)), (ps, pd, 1, H, W, table, _native.ColorLut(17, -1)),
                 (ps, pd, 1, H, W, table, None), (ps, pd, -1, H, W, table, good), (ps, pd, 1, -1, W, table, good),
                 (ps, pd, 1, H, -1, table, good), (None, pd, 1, H, W, table, good), (ps, None, 1, H, W, table, good),
                 (ps, pd, 1, H, W, None, good), (null, pd, 1, H, W, table, good), (ps, null, 1, H, W, table, good)):
        assert L.mi_isp_color_lut_rgb_batch(*args, stream) == 1
        assert b"color_lut" in L.mi_isp_last_error()
        assert L.mi_isp_color_lut_rgb_batch_path(*args, AUTO, stream) == 1
        assert b"color_lut" in L.mi_isp_last_error()
    for path, s in ((3, good), (-1, good), (LDS, _native.ColorLut(34, 64))):
        assert L.mi_isp_color_lut_rgb_batch_path(ps, pd, 1, H, W, table, s, path, stream) == 1
        assert b"color_lut" in L.mi_isp_last_error()
    assert L.mi_isp_color_lut_rgb_batch(ps, pd, 0, H, W, table, good, stream) == 0
    assert L.mi_isp_color_lut_rgb_batch(ps, pd, 1, 0, W, table, good, stream) == 0
    assert L.mi_isp_color_lut_rgb_batch(ps, pd, 1, H, 0, table, good, stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((dst == 99).all())
    assert_exact(src.cpu().numpy(), img, "the source")
    assert L.mi_isp_color_lut_rgb_batch(ps, pd, 1, H, W, table, good, stream) == 0
    ref = C.color_lut_rgb(img, lut.table)
    assert not np.array_equal(ref, img)
    assert_exact(dst.cpu().numpy(), ref, "the good call")


def test_containers(ti, dev):
    img = C.gpu_images(31, 33)["scene"]
    lut = ti.ColorLut(C.gpu_tables(17)["look"], 0.75)
    ref = C.color_lut_rgb(img, lut.table, 0.75)
    assert not np.array_equal(ref, img)
    host = ti.color_lut.apply_lut(img, lut)                           # numpy in, numpy out
    assert isinstance(host, np.ndarray) and host is not img
    assert_exact(host, ref, "numpy")
    cpu_in = torch.from_numpy(img.copy())
    cpu = ti.color_lut.apply_lut(cpu_in, lut)                         # torch on the CPU comes back on the CPU
    assert isinstance(cpu, torch.Tensor) and cpu.device.type == "cpu" and cpu.data_ptr() != cpu_in.data_ptr()
    assert_exact(cpu.numpy(), ref, "torch cpu")
    assert_exact(cpu_in.numpy(), img, "the input")
    flipped = torch.from_numpy(img).to(dev).flip(1)                   # (not contiguous)
    assert_exact(ti.color_lut.apply_lut(flipped, lut).cpu().numpy(), C.color_lut_rgb(np.ascontiguousarray(img[:, ::-1]), lut.table, 0.75),
                 "a view")
    f32 = ti.ColorLut(C.gpu_tables(17)["look"].astype(np.float32) / 255.0, 0.75)      # a float table: the same codes
    assert_exact(ti.color_lut.apply_lut(img, f32), ref, "float table")
    with pytest.raises(ValueError):
        ti.color_lut.apply_lut(img.astype(np.float32), lut)
    with pytest.raises(ValueError):
        ti.color_lut.apply_lut(img[..., 0], lut)
    with pytest.raises(ValueError):
        ti.color_lut.apply_lut(img, lut.table)
    empty = ti.color_lut.apply_lut(np.zeros((0, 8, 3), np.uint8), lut)
    assert empty.shape == (0, 8, 3)
    assert lut._device_table(dev) is lut._device_table(dev), "the packed table is made once per device"


# ---- through the ISP ------------------------------------------------------------------------------------------------------
LUT_N, LUT_STRENGTH = 17, 0.75
CDN_ARGS = (2, 8, 12, 1.0)
SHARP_ARGS = (1.5, 2, 1, 10)
LC_ARGS = ((2, 3), 2.0, 0.75)
ISP_CASES = ["reinhard", "reinhard_keep", "linear", "only", "process", "process_keep", "rotate_90", "resize"]


def the_lut(ti):
    return ti.ColorLut(C.gpu_tables(LUT_N)["look"], LUT_STRENGTH)


def lut_ref(img):
    return C.color_lut_rgb(img, C.gpu_tables(LUT_N)["look"], LUT_STRENGTH)


def isp_pair(ti, dev, cam, on=True, **kw):
    kw = dict(moving_alpha=0.3, device=dev, **kw)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    mapped = getattr(ti, cam)(ti.BayerPattern.RGGB, color_lut=the_lut(ti) if on else None, **kw)
    return plain, mapped


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
    if case == "rotate_90":
        return dict(transform=ti.ImageTransform[case])
    return dict(resize_width=48) if case == "resize" else {}


def frames_of(rng, dev, H, W, n):
    return [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(n)]


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("case", ISP_CASES)
def test_isp_outputs_are_the_lut_of_the_plain_outputs(ti, rng, dev, monkeypatch, cam, case):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 3)
    plain, mapped = isp_pair(ti, dev, cam, **isp_kwargs(ti, case))
    group = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard")
    for step in range(2):
        want, want_imgs = run_case(ti, plain, case, frames)
        got, got_imgs = run_case(ti, mapped, case, frames)
        what = f"{cam} {case} step {step}"
        for k, (g, w) in enumerate(zip(got, want)):
            ref = lut_ref(w.cpu().numpy())
            assert not np.array_equal(ref, w.cpu().numpy()), what
            assert_exact(g.cpu().numpy(), ref, f"{what} output {k}")
        assert_exact(mapped.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), what + " metering state")
        if want_imgs is not None:
            for k, (g, w) in enumerate(zip(got_imgs, want_imgs)):
                assert_exact(g.cpu().numpy(), w.cpu().numpy(), f"{what} image {k}")
    if case in ("process", "process_keep"):           # Camera16 takes the one-launch camera group, Camera32 the two calls
        assert len(group) == (4 if cam == "Camera16" else 0), f"{cam}: {len(group)} camera-group launches"


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("H,W", [(64, 96), (66, 100)])
def test_isp_yuv420_converts_the_lut_of_the_rgb_outputs(ti, rng, dev, monkeypatch, cam, H, W):
    """With a LUT the fused YUV store is never taken (W = 96 would take it): the output is rgb_yuv420_image of the LUT of
    the plain RGB output, then the planar operators."""
    frames = frames_of(rng, dev, H, W, 2)
    plain, mapped = isp_pair(ti, dev, cam)
    both = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev, color_lut=the_lut(ti),
                            sharpen=ti.Sharpen(*SHARP_ARGS))
    fused = _count_calls(monkeypatch, "mi_isp_reinhard_batch_yuv420")
    for step in range(2):
        want, want_imgs = run_case(ti, plain, "reinhard", frames)
        got, got_imgs = run_case(ti, mapped, "yuv420", frames)
        got_sharp, _ = run_case(ti, both, "yuv420", frames)
        for k, (g, gs, w) in enumerate(zip(got, got_sharp, want)):
            mapped_rgb = lut_ref(w.cpu().numpy())
            ref = ti.color.rgb_yuv420_image(torch.from_numpy(mapped_rgb).to(dev)).cpu().numpy()
            assert not np.array_equal(ref, ti.color.rgb_yuv420_image(w).cpu().numpy())
            assert_exact(g.cpu().numpy(), ref, f"{cam} yuv420 {H}x{W} step {step} output {k}")
            assert_exact(gs.cpu().numpy(), S.sharpen_yuv420(ref, *SHARP_ARGS), f"{cam} yuv420 + sharpen, output {k}")
        assert_exact(mapped.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), "metering state")
        for g, w in zip(got_imgs, want_imgs):
            assert_exact(g.cpu().numpy(), w.cpu().numpy(), "images")
    assert not fused


@pytest.mark.parametrize("cam", CAMS)
def test_the_order_is_lut_then_denoise_then_local_contrast_then_sharpen(ti, rng, dev, cam):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 2)
    kw = dict(moving_alpha=0.3, device=dev)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    full = getattr(ti, cam)(ti.BayerPattern.RGGB, color_lut=the_lut(ti), chroma_denoise=ti.ChromaDenoise(*CDN_ARGS),
                            local_contrast=ti.LocalContrast(*LC_ARGS), sharpen=ti.Sharpen(*SHARP_ARGS), **kw)

    def rest(x):
        return S.sharpen_rgb(R.clahe_rgb(CD.chroma_denoise_rgb(x, *CDN_ARGS), *LC_ARGS), *SHARP_ARGS)

    for case in ("reinhard", "process", "linear"):
        want, _ = run_case(ti, plain, case, frames)
        got, _ = run_case(ti, full, case, frames)
        for g, w in zip(got, want):
            w = w.cpu().numpy()
            ref = rest(lut_ref(w))
            assert_exact(g.cpu().numpy(), ref, f"{cam} {case}")
            assert not np.array_equal(ref, lut_ref(rest(w))), "the order shows"
            assert not np.array_equal(ref, rest(w))


def test_set_turns_it_on_and_off(ti, rng, dev):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 1)
    plain, isp = isp_pair(ti, dev, "Camera32", on=False)
    assert isp.color_lut is None
    lut = the_lut(ti)

    def step():
        want = plain.tonemap_reinhard(plain.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()
        return want, isp.tonemap_reinhard(isp.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()

    want, got = step()
    assert_exact(got, want, "off")
    isp.set(color_lut=lut)
    assert isp.color_lut is lut
    want, got = step()
    assert_exact(got, lut_ref(want), "on with the next call")
    isp.set(moving_alpha=0.3)                                          # (None leaves it)
    assert isp.color_lut is lut
    other = ti.ColorLut(C.gpu_tables(33)["random"], 0.5)
    isp.set(color_lut=other)
    assert isp.color_lut is other
    want, got = step()
    ref = C.color_lut_rgb(want, other.table, 0.5)
    assert not np.array_equal(ref, lut_ref(want))
    assert_exact(got, ref, "replaced")
    isp.set(color_lut=False)
    assert isp.color_lut is None
    want, got = step()
    assert_exact(got, want, "off again")
    with pytest.raises(ValueError):
        isp.set(color_lut=1.0)
    with pytest.raises(ValueError):
        isp.set(color_lut=C.gpu_tables(17)["look"])


@pytest.mark.parametrize("cam", CAMS)
def test_without_a_color_lut_no_new_entry_point_is_called(ti, rng, dev, monkeypatch, cam):
    H, W = 64, 96
    frames = frames_of(rng, dev, H, W, 2)
    counts = [_count_calls(monkeypatch, name) for name in ENTRY_POINTS]
    fused = _count_calls(monkeypatch, "mi_isp_reinhard_batch_yuv420")
    for case in ISP_CASES + ["yuv420"]:
        isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, sharpen=ti.Sharpen(), local_contrast=ti.LocalContrast((2, 2)),
                               chroma_denoise=ti.ChromaDenoise(), **isp_kwargs(ti, case))
        assert isp.color_lut is None
        run_case(ti, isp, case, frames)
        assert not counts[0] and not counts[1], case
    assert len(fused) == 1, "the fused YUV entry point is still taken"
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, color_lut=the_lut(ti))      # (the probe does count)
    run_case(ti, isp, "reinhard", frames)
    run_case(ti, isp, "yuv420", frames)
    assert len(counts[0]) == 2 and not counts[1] and len(fused) == 1


def test_graph_capture_of_a_step(ti, rng, dev):
    """load + tonemap_reinhard with the LUT captured once (a single chain of launches; the table was uploaded when the camera
    was made) and replayed on new frame contents."""
    H, W = 64, 96
    frames = [[torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.02 * ((k + j) % 3))).to(dev)
               for j in range(2)] for k in range(3)]
    static = [torch.empty_like(f) for f in frames[0]]
    cap = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev, color_lut=the_lut(ti))
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
            ref = lut_ref(b.cpu().numpy())
            assert not np.array_equal(ref, b.cpu().numpy())
            assert_exact(a.cpu().numpy(), ref, f"replay {k}")
        seen.append(outs[0].cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]), "the replays saw the same frame"
