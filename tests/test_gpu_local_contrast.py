"""Local contrast (Camera16/32 local_contrast=, clahe, clahe_yuv420) on the GPU against tests/local_contrast_ref.py, bit for
bit.  Through the ISP, the output with local contrast must be the restatement applied to the output of an identical ISP
without it, with the same metering state and the same mutated images."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import local_contrast_ref as R
from tests import sharpen_ref as S
from tests.util import _count_calls, assert_exact, natural_packed12, u8_batch_with_sentinels

pytestmark = pytest.mark.gpu

CAMS = ["Camera16", "Camera32"]
CLIPS = [None, 1.0, 2.0, 4.0]
STRENGTHS = [1.0, 0.5, 0.0]
# (H, W), tiles, extra clip limits, inputs
CASES = [
    ((1, 1), (1, 1), [], ["random", "scene"]),                    # the smallest frame
    ((16, 16), (16, 16), [], ["random", "scene"]),                # one-pixel tiles
    ((37, 53), (3, 4), [], ["random", "scene"]),                  # boundaries that do not divide
    ((70, 260), (2, 3), [], ["random", "scene"]),                 # crosses an apply block in both axes
    ((130, 140), (8, 8), [], ["random", "scene"]),                # many LUTs per block
    ((130, 140), (16, 16), [], ["scene"]),                        # more 2 x 2 cells than a block keeps in LDS
    ((400, 520), (2, 2), [], ["random", "scene"]),                # several histogram work-groups per tile
    ((300, 300), (1, 1), [], ["flat"]),                           # 90 000 pixels in one bin: a 16-bit counter overflows
    ((512, 512), (1, 1), [64.0], ["random", "scene"]),            # C n passes 2^32
    ((2904, 2900), (1, 1), [], ["random", "scene"]),              # 510 cdf passes 2^32
]
ENTRY_POINTS = ("mi_isp_local_contrast_rgb_batch", "mi_isp_local_contrast_yuv420_batch")


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_input(rng, kind, H, W):
    if kind == "flat":
        return np.full((H, W, 3), 100, np.uint8)
    if kind == "random":
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif H * W > 1 << 20:                                          # (the scene at a quarter of the size, every pixel 4 x 4)
        img = np.repeat(np.repeat(S.scene_u8(rng, H // 4, W // 4), 4, axis=0), 4, axis=1)
    else:
        img = S.scene_u8(rng, H, W)
    if H * W > 1 << 20:
        img[0, :8] = 255                                           # (the largest cdf values are read)
    return img


def same(got, ref, what):
    """got (a device tensor) is ref (numpy), compared on the device; the first difference is named on a mismatch."""
    if not torch.equal(got, torch.from_numpy(ref).to(got.device)):
        assert_exact(got.cpu().numpy(), ref, what)


# ---- the operator on its own -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,tiles,more_clips,kind",
                         [pytest.param(s, t, c, k, id=f"{s[0]}x{s[1]}-{t[0]}x{t[1]}-{k}")
                          for s, t, c, kinds in CASES for k in kinds])
def test_clahe_against_the_restatement(ti, rng, dev, shape, tiles, more_clips, kind):
    """RGB and, on the luma plane of the same image (H even; a chroma block of another value under it), the Y-plane form:
    E of the restatement is computed once per clip limit."""
    H, W = shape
    img = make_input(rng, kind, H, W)
    L = S.luma(img)
    t = torch.from_numpy(img).to(dev)
    yuv = None
    if H % 2 == 0 and W % 2 == 0:
        yuv = np.concatenate([L.astype(np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)])
        ty = torch.from_numpy(yuv).to(dev)
    refs = {}
    for clip in CLIPS + more_clips:
        E = R.equalised(L, tiles, clip)
        for strength in STRENGTHS:
            lc = ti.LocalContrast(tiles, clip, strength)
            dl = R.blend(E, L, strength)
            what = f"{kind} {H}x{W} tiles {tiles} clip {clip} strength {strength}"
            ref = R.add_rgb(img, dl)
            got = ti.local_contrast.clahe(t, lc)
            assert isinstance(got, torch.Tensor) and got.device == dev and got.data_ptr() != t.data_ptr()
            same(got, ref, what)
            refs[clip, strength] = ref
            if yuv is not None:
                same(ti.local_contrast.clahe_yuv420(ty, lc), R.add_yuv420(yuv, dl), "yuv " + what)
        if clip == 2.0 and kind != "flat" and H * W >= 37 * 53:      # floor and truncation must differ on this input
            assert not np.array_equal(R.blend(E, L, 0.5, truncate=True), R.blend(E, L, 0.5)), "no delta that truncation moves"
    same(t, img, "the input is left alone")
    if H * W >= 37 * 53:
        check_not_vacuous(img, refs, CLIPS + more_clips, kind, tiles, f"{kind} {H}x{W}")


def check_not_vacuous(img, refs, clips, kind, tiles, what):
    """Every strength > 0 moves the input, strength 0 is the identity, and the references of the clip limits differ from
    each other where their ceilings c = max(1, (C n) >> 16) do (tiles of fewer than 256 pixels have c = 1 up to clip 2).  The
    flat image at clip 1 has E - L = 1 everywhere, which strength 0.5 rounds to 1 again."""
    n = (img.shape[0] // tiles[0]) * (img.shape[1] // tiles[1])       # the smallest tile
    for clip in clips:
        assert np.array_equal(refs[clip, 0.0], img), f"{what}: strength 0 is not the identity"
        assert not np.array_equal(refs[clip, 1.0], img), f"{what}: clip {clip} leaves the input as it is"
        if not (kind == "flat" and clip == 1.0):
            assert not np.array_equal(refs[clip, 0.5], refs[clip, 1.0]), f"{what}: strength 0.5 is strength 1"
    for a, b in zip(clips, clips[1:]):
        if a is not None and kind == "random":                       # (no bin of a random image holds twice the uniform share)
            continue
        if a is not None and max(1, (R.clip_q8(a) * n) >> 16) == max(1, (R.clip_q8(b) * n) >> 16):
            continue
        assert not np.array_equal(refs[a, 1.0], refs[b, 1.0]), f"{what}: clip {a} and clip {b} give the same output"


def test_the_restatement_in_one_call_is_the_restatement_in_pieces(rng):
    """clahe_rgb / clahe_yuv420 of the restatement are the pieces the test above composes."""
    img = S.scene_u8(rng, 38, 54)
    L = S.luma(img)
    dl = R.blend(R.equalised(L, (3, 4), 2.0), L, 0.5)
    assert np.array_equal(R.clahe_rgb(img, (3, 4), 2.0, 0.5), R.add_rgb(img, dl))
    yuv = np.concatenate([L.astype(np.uint8), np.full((19, 54), 9, np.uint8)])
    assert np.array_equal(R.clahe_yuv420(yuv, (3, 4), 2.0, 0.5), R.add_yuv420(yuv, dl))


def test_containers(ti, rng, dev):
    img = S.scene_u8(rng, 38, 54)
    lc = ti.LocalContrast((3, 4), 2.0, 0.75)
    ref = R.clahe_rgb(img, (3, 4), 2.0, 0.75)
    assert not np.array_equal(ref, img)
    host = ti.local_contrast.clahe(img, lc)                          # numpy in, numpy out
    assert isinstance(host, np.ndarray) and host is not img
    assert_exact(host, ref, "numpy")
    cpu = ti.local_contrast.clahe(torch.from_numpy(img), lc)         # torch on the CPU comes back on the CPU
    assert isinstance(cpu, torch.Tensor) and cpu.device.type == "cpu"
    assert_exact(cpu.numpy(), ref, "torch cpu")
    yuv = rng.integers(0, 256, (9, 10)).astype(np.uint8)
    host = ti.local_contrast.clahe_yuv420(yuv, lc)
    assert isinstance(host, np.ndarray)
    assert_exact(host, R.clahe_yuv420(yuv, (3, 4), 2.0, 0.75), "numpy yuv")
    with pytest.raises(ValueError):
        ti.local_contrast.clahe(img.astype(np.float32), lc)
    with pytest.raises(ValueError):
        ti.local_contrast.clahe(img, ((3, 4), 2.0))
    with pytest.raises(ValueError):                                  # fewer rows than tile rows
        ti.local_contrast.clahe(img[:2], lc)
    with pytest.raises(ValueError):
        ti.local_contrast.clahe(img[:, :3], lc)
    empty = ti.local_contrast.clahe(np.zeros((0, 8, 3), np.uint8), lc)
    assert empty.shape == (0, 8, 3)


@pytest.mark.parametrize("H,W", [(64, 64), (37, 53)])
def test_views_at_odd_byte_offsets_take_the_byte_path(ti, rng, dev, H, W):
    """An image that starts 1, 2 or 3 bytes past a 4-byte boundary (W % 4 == 0 at 64 x 64: only the base is odd), RGB and
    plane."""
    img = S.scene_u8(rng, H, W)
    lc = ti.LocalContrast((3, 4), 2.0, 0.75)
    ref = R.clahe_rgb(img, (3, 4), 2.0, 0.75)
    assert not np.array_equal(ref, img)
    n = H * W * 3
    buf = torch.zeros(n + 8, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        view = buf[off:off + n].view(H, W, 3)
        view.copy_(torch.from_numpy(img))
        assert view.data_ptr() % 4 == (buf.data_ptr() + off) % 4 != 0
        assert_exact(ti.local_contrast.clahe(view, lc).cpu().numpy(), ref, f"offset {off}")
        ti.local_contrast.apply([view], lc, inplace=True)            # (an odd destination too)
        assert_exact(view.cpu().numpy(), ref, f"offset {off} in place")
    if H % 2 == 0:
        yuv = np.concatenate([S.luma(img).astype(np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)])
        ref = R.clahe_yuv420(yuv, (3, 4), 2.0, 0.75)
        for off in (1, 2, 3):
            view = buf[off:off + yuv.size].view(*yuv.shape)
            view.copy_(torch.from_numpy(yuv))
            assert_exact(ti.local_contrast.clahe_yuv420(view, lc).cpu().numpy(), ref, f"yuv offset {off}")


@pytest.mark.parametrize("n", [1, 3, 33])
def test_batches(ti, rng, dev, n):
    """33 images cross the 32-per-launch split."""
    H, W = 16, 20
    imgs = [S.scene_u8(rng, H, W, sigma=0.03 + 0.002 * k) for k in range(n)]
    lc = ti.LocalContrast((2, 3), 2.0, 0.75)
    outs = ti.local_contrast.apply([torch.from_numpy(i).to(dev) for i in imgs], lc)
    assert len(outs) == n
    for k in range(n):
        ref = R.clahe_rgb(imgs[k], (2, 3), 2.0, 0.75)
        assert not np.array_equal(ref, imgs[k])
        assert_exact(outs[k].cpu().numpy(), ref, f"image {k} of {n}")
    yuvs = [rng.integers(0, 256, (H * 3 // 2, W)).astype(np.uint8) for _ in range(n)]
    outs = ti.local_contrast.apply([torch.from_numpy(y).to(dev) for y in yuvs], lc, yuv420=True)
    for k in range(n):
        assert_exact(outs[k].cpu().numpy(), R.clahe_yuv420(yuvs[k], (2, 3), 2.0, 0.75), f"yuv image {k} of {n}")


@pytest.mark.parametrize("H,W", [(8, 16), (6, 10)])
def test_the_second_launch_group(ti, rng, dev, H, W):
    """33 images of distinct contents through the entry points themselves, on the dword path (8 x 16) and on the byte path
    (6 x 10), none filtered in place and every second one: image 32 is the second group of 32 - the second part of the
    workspace - and, for the planar form, the second copy of the chroma rows, which takes only the images not filtered in
    place.  Sentinel bytes behind every destination."""
    from taichi_image_amd import _native
    tiles, clip, strength = (2, 3), 2.0, 0.75
    arg = ti.LocalContrast(tiles, clip, strength)._arg()
    ws = torch.empty(int(_native.lib().mi_isp_local_contrast_workspace_bytes(33, arg)), dtype=torch.uint8, device=dev)
    imgs = [S.scene_u8(rng, H, W, sigma=0.03 + 0.002 * k) for k in range(33)]
    yuvs = [rng.integers(0, 256, (H * 3 // 2, W)).astype(np.uint8) for _ in range(33)]
    refs = [R.clahe_rgb(i, tiles, clip, strength) for i in imgs]
    yuv_refs = [R.clahe_yuv420(y, tiles, clip, strength) for y in yuvs]
    assert not np.array_equal(refs[32], imgs[32]) and not np.array_equal(refs[32], refs[0])
    assert not np.array_equal(yuv_refs[32], yuvs[32])
    for in_place in ((), range(0, 33, 2), range(1, 33, 2)):
        outs = u8_batch_with_sentinels(ENTRY_POINTS[0], imgs, H, W, (arg, ws.data_ptr()), dev, in_place)
        for k in range(33):
            assert_exact(outs[k], refs[k], f"{H}x{W} image {k}, in place: {list(in_place)[:2]}")
        outs = u8_batch_with_sentinels(ENTRY_POINTS[1], yuvs, H, W, (arg, ws.data_ptr()), dev, in_place)
        for k in range(33):
            assert_exact(outs[k], yuv_refs[k], f"{H}x{W} yuv image {k}, in place: {list(in_place)[:2]}")


def test_in_place(ti, rng, dev):
    """src == dst, RGB and YUV (whose chroma rows then stay where they are), one image of a batch and all of them."""
    H, W = 70, 132
    imgs = [S.scene_u8(rng, H, W, sigma=0.03 + 0.01 * k) for k in range(3)]
    lc = ti.LocalContrast((2, 3), 2.0, 1.0)
    ts = [torch.from_numpy(i).to(dev) for i in imgs]
    ptrs = [t.data_ptr() for t in ts]
    outs = ti.local_contrast.apply(ts, lc, inplace=True)
    assert [o.data_ptr() for o in outs] == ptrs
    for k in range(3):
        assert_exact(ts[k].cpu().numpy(), R.clahe_rgb(imgs[k], (2, 3), 2.0, 1.0), f"image {k}")
    yuvs = [rng.integers(0, 256, (H * 3 // 2, W)).astype(np.uint8) for _ in range(2)]
    ts = [torch.from_numpy(y).to(dev) for y in yuvs]
    ti.local_contrast.apply(ts, lc, yuv420=True, inplace=True)
    for k in range(2):
        assert_exact(ts[k].cpu().numpy(), R.clahe_yuv420(yuvs[k], (2, 3), 2.0, 1.0), f"yuv image {k}")
    # through the C entry point: image 0 in place, image 1 into another buffer whose chroma rows are copied
    from taichi_image_amd import _native
    L = _native.lib()
    ts = [torch.from_numpy(y).to(dev) for y in yuvs]
    other = torch.zeros_like(ts[1])
    arg = lc._arg()
    ws = torch.empty(int(L.mi_isp_local_contrast_workspace_bytes(2, arg)), dtype=torch.uint8, device=dev)
    assert L.mi_isp_local_contrast_yuv420_batch(_native.ptr_array(ts), _native.ptr_array([ts[0], other]), 2, H, W, arg,
                                                ws.data_ptr(), _native.stream_ptr(dev)) == 0
    assert_exact(ts[0].cpu().numpy(), R.clahe_yuv420(yuvs[0], (2, 3), 2.0, 1.0), "in place")
    assert_exact(other.cpu().numpy(), R.clahe_yuv420(yuvs[1], (2, 3), 2.0, 1.0), "out of place")
    assert_exact(ts[1].cpu().numpy(), yuvs[1], "the source of the out-of-place image")


# ---- through the ISP ------------------------------------------------------------------------------------------------------
# (2 x 3 tiles of a 64 x 96 output: 12 LUT cells under one apply block, which keeps them in LDS)
LC = dict(tiles=(2, 3), clip_limit=2.0, strength=0.75)
LC_ARGS = ((2, 3), 2.0, 0.75)
SHARP = dict(amount=1.5, radius=2, threshold=1, overshoot=10)
SHARP_ARGS = (1.5, 2, 1, 10)
ISP_CASES = ["reinhard", "reinhard_keep", "linear", "only", "process", "process_keep", "rotate_90", "flip_horiz", "resize"]


def isp_pair(ti, dev, cam, sharpen=False, **kw):
    kw = dict(moving_alpha=0.3, device=dev, **kw)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    both = getattr(ti, cam)(ti.BayerPattern.RGGB, local_contrast=ti.LocalContrast(**LC),
                            sharpen=ti.Sharpen(**SHARP) if sharpen else None, **kw)
    return plain, both


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


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("sharpen", [False, True])
@pytest.mark.parametrize("case", ISP_CASES)
def test_isp_outputs_are_the_operator_of_the_plain_outputs(ti, rng, dev, monkeypatch, cam, sharpen, case):
    """With sharpen= set too, the output is sharpen(local_contrast(x)).  The tile grid is that of the returned image
    (rotate_90 returns 96 x 64)."""
    H, W = 64, 96
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(3)]
    plain, both = isp_pair(ti, dev, cam, sharpen=sharpen, **isp_kwargs(ti, case))
    group = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard")
    for step in range(2):
        want, want_imgs = run_case(ti, plain, case, frames)
        got, got_imgs = run_case(ti, both, case, frames)
        what = f"{cam} {case} sharpen {sharpen} step {step}"
        for k, (g, w) in enumerate(zip(got, want)):
            w = w.cpu().numpy()
            ref = R.clahe_rgb(w, *LC_ARGS)
            assert not np.array_equal(ref, w), what
            if sharpen:
                ref, before = S.sharpen_rgb(ref, *SHARP_ARGS), ref
                assert not np.array_equal(ref, before), what
                assert not np.array_equal(ref, R.clahe_rgb(S.sharpen_rgb(w, *SHARP_ARGS), *LC_ARGS)), what + ": the order shows"
            assert_exact(g.cpu().numpy(), ref, f"{what} output {k}")
        assert_exact(both.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), what + " metering state")
        if want_imgs is not None:
            for k, (g, w) in enumerate(zip(got_imgs, want_imgs)):
                assert_exact(g.cpu().numpy(), w.cpu().numpy(), f"{what} image {k}")
    if case in ("process", "process_keep"):           # Camera16 takes the one-launch camera group, Camera32 the two calls
        assert len(group) == (4 if cam == "Camera16" else 0), f"{cam}: {len(group)} camera-group launches"


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("H,W,fused", [(64, 96, True), (66, 100, False)])
def test_isp_yuv420_equalises_the_y_plane(ti, rng, dev, monkeypatch, cam, H, W, fused):
    """W % 16 == 0 takes the fused YUV store, W = 100 the RGB tonemap and the separate conversion: either way the output is
    the Y-plane operator of the plain call's YUV image (not the YUV image of the RGB result)."""
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(2)]
    calls = _count_calls(monkeypatch, "mi_isp_reinhard_batch_yuv420")
    rgb_calls = _count_calls(monkeypatch, "mi_isp_local_contrast_rgb_batch")
    for sharpen in (False, True):
        plain, both = isp_pair(ti, dev, cam, sharpen=sharpen)
        for step in range(2):
            want, want_imgs = run_case(ti, plain, "yuv420", frames)
            got, got_imgs = run_case(ti, both, "yuv420", frames)
            for k, (g, w) in enumerate(zip(got, want)):
                ref = R.clahe_yuv420(w.cpu().numpy(), *LC_ARGS)
                assert not np.array_equal(ref, w.cpu().numpy())
                if sharpen:
                    ref = S.sharpen_yuv420(ref, *SHARP_ARGS)
                assert_exact(g.cpu().numpy(), ref, f"{cam} yuv420 {H}x{W} sharpen {sharpen} step {step} output {k}")
            assert_exact(both.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), "metering state")
            for g, w in zip(got_imgs, want_imgs):
                assert_exact(g.cpu().numpy(), w.cpu().numpy(), "images")
    assert len(calls) == (8 if fused else 0) and not rgb_calls


def test_set_turns_it_on_and_off(ti, rng, dev):
    H, W = 64, 96
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB)).to(dev)]
    plain = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    assert isp.local_contrast is None
    lc = ti.LocalContrast(**LC)

    def step():
        want = plain.tonemap_reinhard(plain.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()
        return want, isp.tonemap_reinhard(isp.load_packed12_batch(frames), gamma=0.7)[0].cpu().numpy()

    want, got = step()
    assert_exact(got, want, "off")
    isp.set(local_contrast=lc)
    assert isp.local_contrast == lc
    want, got = step()
    assert_exact(got, R.clahe_rgb(want, *LC_ARGS), "on with the next call")
    isp.set(moving_alpha=0.3)                                          # (None leaves it)
    assert isp.local_contrast == lc
    isp.set(local_contrast=ti.LocalContrast((2, 2), None, 0.5))
    want, got = step()
    assert_exact(got, R.clahe_rgb(want, (2, 2), None, 0.5), "replaced")
    isp.set(local_contrast=False)
    assert isp.local_contrast is None
    want, got = step()
    assert_exact(got, want, "off again")
    with pytest.raises(ValueError):
        isp.set(local_contrast=1.0)
    isp.set(local_contrast=ti.LocalContrast((16, 16)), resize_width=12)  # 8 x 12 outputs: fewer rows than tile rows
    before = isp.metrics.clone()
    with pytest.raises(ValueError):                                    # refused before the tonemap moves the metering state
        step()
    assert_exact(isp.metrics.cpu().numpy(), before.cpu().numpy(), "metering state after the refused call")
    imgs = isp.load_packed12_batch(frames)
    for call in (lambda: isp.tonemap_linear(imgs), lambda: isp.tonemap_reinhard_yuv420(imgs),
                 lambda: isp.tonemap_only(imgs[0], isp.metrics, 0.7, 1.0, 1.0, 0.0), lambda: isp.process_packed12(frames)):
        with pytest.raises(ValueError):
            call()
    assert_exact(isp.metrics.cpu().numpy(), before.cpu().numpy(), "metering state after the refused calls")


@pytest.mark.parametrize("cam", CAMS)
def test_without_local_contrast_no_new_entry_point_is_called(ti, rng, dev, monkeypatch, cam):
    H, W = 64, 96
    frames = [torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.03 * k)).to(dev) for k in range(2)]
    counts = [_count_calls(monkeypatch, name) for name in ENTRY_POINTS + ("mi_isp_local_contrast_workspace_bytes",)]
    for case in ISP_CASES + ["yuv420"]:
        for sharpen in (None, ti.Sharpen()):
            isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, sharpen=sharpen, **isp_kwargs(ti, case))
            run_case(ti, isp, case, frames)
            assert not any(counts), case
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, local_contrast=ti.LocalContrast())      # (the probe does count)
    run_case(ti, isp, "reinhard", frames)
    run_case(ti, isp, "yuv420", frames)
    assert [len(c) for c in counts] == [1, 1, 2]


def test_graph_capture_of_a_step(ti, rng, dev):
    """load + tonemap_reinhard with local contrast captured once and replayed on new frame contents."""
    H, W = 64, 96
    frames = [[torch.from_numpy(natural_packed12(rng, H, W, O.RGGB, dark=0.02 * ((k + j) % 3))).to(dev)
               for j in range(2)] for k in range(3)]
    static = [torch.empty_like(f) for f in frames[0]]
    cap = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev, local_contrast=ti.LocalContrast(**LC))
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
            assert_exact(a.cpu().numpy(), R.clahe_rgb(b.cpu().numpy(), *LC_ARGS), f"replay {k}")
        seen.append(outs[0].cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]), "the replays saw the same frame"


# ---- C ABI error returns ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_without_a_launch(ti, dev):
    """Bad tiles, a frame smaller than its grid and a missing workspace are refused by the host checks: the destination
    stays as it was; n = 0 succeeds and launches nothing."""
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = 8, 12
    src = torch.full((H, W, 3), 7, dtype=torch.uint8, device=dev)
    src[:, ::2] = 200
    dst = torch.full((H, W, 3), 99, dtype=torch.uint8, device=dev)
    good = _native.LocalContrast(2, 2, 512, 64)
    ws = torch.empty(int(L.mi_isp_local_contrast_workspace_bytes(1, good)), dtype=torch.uint8, device=dev)
    stream = _native.stream_ptr(dev)
    for fn in (L.mi_isp_local_contrast_rgb_batch, L.mi_isp_local_contrast_yuv420_batch):
        for args in ((1, H, W, _native.LocalContrast(2, 17, 512, 64), ws.data_ptr()),
                     (1, H, W, _native.LocalContrast(9, 2, 512, 64), ws.data_ptr()),
                     (1, H, W, good, None)):
            assert fn(_native.ptr_array([src]), _native.ptr_array([dst]), *args, stream) == 1
            assert b"local_contrast" in L.mi_isp_last_error()
        assert fn(_native.ptr_array([src]), _native.ptr_array([dst]), 0, H, W, good, ws.data_ptr(), stream) == 0
    torch.cuda.synchronize(dev)
    assert bool((dst == 99).all()) and int(src[0, 0, 0]) == 200
    assert L.mi_isp_local_contrast_rgb_batch(_native.ptr_array([src]), _native.ptr_array([dst]), 1, H, W, good,
                                             ws.data_ptr(), stream) == 0
    assert_exact(dst.cpu().numpy(), R.clahe_rgb(src.cpu().numpy(), (2, 2), 2.0, 1.0), "the good call")
