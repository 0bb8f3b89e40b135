"""Auto white balance (Camera16/32 auto_white_balance=) on the GPU against the contract.

Expected values come from the NumPy restatement (tests/awb_ref.py) and the existing oracle: every step's statistics
from the pre-cast values x and the user's gains, the gains after each update, and the images loaded through the
effective grid E (O.cast_out, O.bayer_to_rgb, O.resize_bilinear through the lens shading tests' helpers).  Step k's
loads use the gains after step k-1's update; the first step uses the seed f32(white_balance).
"""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import awb_ref as A
from tests.test_gpu_shading import make_grid, pixel_gains, raw_x, ref_load
from tests.util import assert_exact

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
PER_SITE = [64, 200, 180, 256]
WB = np.array([1.8, 1.0, 2.1])
H, W = 64, 128
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def scene_codes(rng, h, w, pattern, cast, top):
    """Raw codes (h, w) of a smooth scene with colour cast `cast` (r, g, b), mosaiced under `pattern`."""
    r = np.arange(h)[:, None] / h
    c = np.arange(w)[None, :] / w
    base = 0.05 + 0.9 * (0.5 + 0.5 * np.sin(5.0 * r + 1.0)) * (0.5 + 0.5 * np.cos(7.0 * c))
    img = np.stack([np.clip(base * g + rng.normal(0, 0.02, (h, w)), 0, 1) for g in cast], -1)
    cfa = O.rgb_to_bayer(img.astype(f32), pattern)
    return np.rint(cfa.astype(np.float64) * top).astype(np.uint16)


def pack(codes, layout):
    if layout == "p16":
        return codes.view(np.uint8).reshape(codes.shape[0], 2 * codes.shape[1])
    return O.encode12(codes, ids_format=layout == "ids")


def decoded(codes, layout):
    """The codes the loader reads back from pack(codes, layout) (the IDS packing of O.encode12 does not round-trip)."""
    return codes if layout == "p16" else O.decode12(pack(codes, layout), "u16", ids_format=layout == "ids")


CASTS = [(1.0, 0.8, 0.6), (0.6, 0.9, 1.0), (0.9, 0.7, 0.8)]


def user_grid(rng, kind):
    return None if kind == "none" else make_grid(rng, 9, 7, 1 if kind == "1site" else 4)


def ref_steps(frames_codes, bits, layout, work, pattern, user, black, white, alpha, resize_width=0):
    """Per step: the expected images of the step's frames and the gains after its update."""
    st = A.State(WB)
    out = []
    for codes_list in frames_codes:
        E = A.effective(st.gains, pattern, user)
        imgs = [ref_load(pack(c, layout), bits, work, pattern, E, black, white, resize_width, layout == "ids")
                for c in codes_list]
        g = None if user is None else pixel_gains(user, *codes_list[0].shape)
        st.update(A.add(*[A.stats(raw_x(decoded(c, layout), bits, black, white), g) for c in codes_list]), pattern, alpha)
        out.append((imgs, st.gains.copy(), A.effective(st.gains, pattern, user)))
    return out


def check_sub(img, ref, what):
    tag = getattr(img, "_mi_metering_sub", None)
    if tag is not None:
        assert_exact(tag[0].cpu().numpy(), ref[::tag[1], ::tag[1]], what + " metering subsample")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("layout", ["std", "ids", "p16"])
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("grid", ["none", "1site", "4site"])
def test_packed_loads_gains_and_images(ti, rng, dev, cam, work, layout, pattern, levels, grid):
    bits = 16 if layout == "p16" else 12
    top = (1 << bits) - 1
    black, white = (PER_SITE, top - 100) if levels else (None, None)
    user = user_grid(rng, grid)
    frames = [[scene_codes(rng, H, W, pattern, CASTS[(k + j) % 3], top) for j in range(2)] for k in range(3)]
    want = ref_steps(frames, bits, layout, work, pattern, user, black, white, 0.3)
    for batch in (True, False):
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), moving_alpha=0.3, device=dev, black_level=black,
                               white_level=white, lens_shading=user, auto_white_balance=True)
        assert np.array_equal(isp.white_balance_gains.cpu().numpy(), WB.astype(f32))
        for k, codes_list in enumerate(frames):
            srcs = [torch.from_numpy(pack(c, layout)).to(dev) for c in codes_list]
            if batch:
                imgs = (isp.load_packed16_batch(srcs) if bits == 16 else
                        isp.load_packed12_batch(srcs, ids_format=layout == "ids"))
            else:
                imgs = [isp.load_packed16(s) if bits == 16 else isp.load_packed12(s, ids_format=layout == "ids")
                        for s in srcs]
            for im, ref in zip(imgs, want[k][0]):
                what = f"{cam} {layout} p{pattern} {grid} levels={levels} batch={batch} step {k}"
                assert_exact(im.cpu().numpy(), ref, what)
                check_sub(im, ref, what)
            isp.tonemap_reinhard(imgs, write_back=False)
            g = isp.white_balance_gains.cpu().numpy()
            assert g.dtype == f32 and np.array_equal(g, want[k][1]), (batch, k, g, want[k][1])
            assert np.array_equal(isp._awb_E.cpu().numpy(), want[k][2])


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("resize_width", [64, 48])
@pytest.mark.parametrize("layout", ["std", "p16"])
def test_resized_loads(ti, rng, dev, cam, work, resize_width, layout):
    """The fused resize (and, at 48, a scale it does not take) on the effective grid."""
    bits = 16 if layout == "p16" else 12
    user = make_grid(rng, 5, 5, 4)
    frames = [[scene_codes(rng, H, W, 1, CASTS[k], (1 << bits) - 1) for _ in range(2)] for k in range(3)]
    want = ref_steps(frames, bits, layout, work, 1, user, None, None, 0.5, resize_width)
    isp = getattr(ti, cam)(ti.BayerPattern.GRBG, moving_alpha=0.5, device=dev, resize_width=resize_width,
                           lens_shading=user, auto_white_balance=True)
    for k, codes_list in enumerate(frames):
        srcs = [torch.from_numpy(pack(c, layout)).to(dev) for c in codes_list]
        imgs = isp.load_packed16_batch(srcs) if bits == 16 else isp.load_packed12_batch(srcs)
        for im, ref in zip(imgs, want[k][0]):
            assert_exact(im.cpu().numpy(), ref, f"{cam} resize {resize_width} step {k}")
        isp.update_white_balance()
        assert np.array_equal(isp.white_balance_gains.cpu().numpy(), want[k][1])


def convert_x(src, mode, black, white):
    if mode == "16u":
        if black is None:
            return src.astype(f32) / f32(65535.0)
        b = np.tile(np.asarray(black, np.int64).reshape(2, 2), (src.shape[0] // 2, src.shape[1] // 2))
        den = np.tile(np.array([[white - black[0], white - black[1]], [white - black[2], white - black[3]]], f32),
                      (src.shape[0] // 2, src.shape[1] // 2))
        return np.maximum(src.astype(np.int64) - b, 0).astype(f32) / den
    return src.astype(f32)


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("mode,levels", [("16u", False), ("16u", True), ("16f", False), ("32f", False)])
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
@pytest.mark.parametrize("grid", ["none", "1site", "4site"])
def test_convert_loads(ti, rng, dev, cam, work, mode, levels, pattern, grid):
    user = user_grid(rng, grid)
    black, white = (PER_SITE, 60000) if levels else (None, None)
    # load_16f converts codes numerically: a clip and floor in those units
    awb = ti.AutoWhiteBalance(clip=5000.0, floor=50.0) if mode == "16f" else ti.AutoWhiteBalance(stride=2)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), moving_alpha=0.2, device=dev, black_level=black, white_level=white,
                           lens_shading=user, auto_white_balance=awb)
    st = A.State(WB)
    for k in range(3):
        codes = scene_codes(rng, H, W, pattern, CASTS[k], 65535 if mode == "16u" else 4095)
        src = codes.astype(f32) / f32(4095) if mode == "32f" else codes
        x = convert_x(src, mode, black, white)
        E = A.effective(st.gains, pattern, user)
        ref = O.bayer_to_rgb(O.cast_out((x * pixel_gains(E, H, W)).astype(f32), work), pattern)
        load = {"16u": isp.load_16u, "16f": isp.load_16f, "32f": isp.load_32f}[mode]
        got = load(torch.from_numpy(src).to(dev))
        assert_exact(got.cpu().numpy(), ref, f"{cam} {mode} p{pattern} {grid} step {k}")
        g = None if user is None else pixel_gains(user, H, W)
        st.update(A.stats(x, g, awb.clip, awb.floor, awb.stride), pattern, 0.2)
        isp.update_white_balance()
        assert np.array_equal(isp.white_balance_gains.cpu().numpy(), st.gains), (k, st.gains)


@pytest.mark.parametrize("ids", [False, True])
def test_process_packed12_equals_its_two_calls(ti, rng, dev, ids):
    frames = [[torch.from_numpy(pack(scene_codes(rng, H, W, 0, CASTS[(k + j) % 3], 4095), "ids" if ids else "std"))
               .to(dev) for j in range(3)] for k in range(3)]
    one = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev, auto_white_balance=True)
    two = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev, auto_white_balance=True)
    for k in range(3):
        outs, imgs = one.process_packed12(frames[k], gamma=0.8, keep_images=True, ids_format=ids)
        ims2 = two.load_packed12_batch(frames[k], ids_format=ids)
        outs2 = two.tonemap_reinhard(ims2, gamma=0.8)
        for a, b in zip(outs, outs2):
            assert torch.equal(a, b)
        for a, b in zip(imgs, ims2):
            assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"process_packed12 images step {k}")
        assert_exact(one.metrics.cpu().numpy(), two.metrics.cpu().numpy(), "metrics")
        assert torch.equal(one.white_balance_gains, two.white_balance_gains)
    assert not torch.equal(one.white_balance_gains.cpu(), torch.from_numpy(WB.astype(f32)))


@pytest.mark.parametrize("cam", ["Camera16", "Camera32"])
def test_defects_and_undistort_apply_the_effective_grid(ti, rng, dev, cam):
    user = make_grid(rng, 6, 6, 4)
    dm = ti.DefectMap([[3, 4], [20, 61], [41, 100]], (H, W))
    K = np.array([[100.0, 0, W / 2], [0, 100.0, H / 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, [-0.1, 0.02, 0.001, -0.001], (H, W))
    awb = getattr(ti, cam)(ti.BayerPattern.GBRG, moving_alpha=0.4, device=dev, black_level=PER_SITE, white_level=4000,
                           lens_shading=user, auto_white_balance=True)
    plain = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, black_level=PER_SITE, white_level=4000)
    for k in range(3):
        src = torch.from_numpy(pack(scene_codes(rng, H, W, 2, CASTS[k], 4095), "std")).to(dev)
        plain.set(lens_shading=awb._awb_E.cpu().numpy())
        for kw in (dict(defects=dm), dict(undistort=lens), dict(defects=dm, undistort=lens)):
            a = awb.load_packed12(src, **kw)
            b = plain.load_packed12(src, **kw)
            assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"{cam} {kw} step {k}")
        a = awb.load_packed12_batch([src, src], defects=[dm, None], undistort=[None, lens])
        b = plain.load_packed12_batch([src, src], defects=[dm, None], undistort=[None, lens])
        for x, y in zip(a, b):
            assert_exact(x.cpu().numpy(), y.cpu().numpy(), f"{cam} batch step {k}")
        awb.update_white_balance()


def test_set_turns_off_reseeds_and_rebuilds(ti, rng, dev):
    frames = [torch.from_numpy(pack(scene_codes(rng, H, W, 3, CASTS[k], 4095), "std")).to(dev) for k in range(3)]
    isp = ti.Camera32(ti.BayerPattern.BGGR, moving_alpha=0.3, device=dev, correct_colors=True, auto_white_balance=True)
    assert np.array_equal(isp.color_correct_matrix, ti.camera_isp.default_cc)        # no white_balance scaling
    for f in frames:
        isp.tonemap_reinhard([isp.load_packed12(f)])
    # off: exactly an ISP that never had AWB (colour matrix included)
    isp.set(auto_white_balance=False)
    assert isp.white_balance_gains is None and isp.auto_white_balance is None
    fresh = ti.Camera32(ti.BayerPattern.BGGR, moving_alpha=0.3, device=dev, correct_colors=True)
    assert np.array_equal(isp.color_correct_matrix, fresh.color_correct_matrix)
    assert_exact(isp.load_packed12(frames[0]).cpu().numpy(), fresh.load_packed12(frames[0]).cpu().numpy(), "AWB off")
    # on again, then re-seeded through white_balance: the state of a fresh ISP with that seed
    isp.set(auto_white_balance=ti.AutoWhiteBalance(stride=2))
    isp.tonemap_reinhard([isp.load_packed12(frames[1])])
    wb2 = np.array([1.25, 0.9, 1.5])
    isp.set(white_balance=wb2)
    assert np.array_equal(isp.white_balance_gains.cpu().numpy(), wb2.astype(f32))
    assert np.array_equal(isp._awb_E.cpu().numpy(), A.effective(wb2.astype(f32), 3))
    ref = ti.Camera32(ti.BayerPattern.BGGR, moving_alpha=0.3, device=dev, correct_colors=True, white_balance=wb2,
                      auto_white_balance=ti.AutoWhiteBalance(stride=2))
    for f in frames:
        a, b = isp.load_packed12(f), ref.load_packed12(f)
        assert_exact(a.cpu().numpy(), b.cpu().numpy(), "re-seeded")
        isp.update_white_balance()
        ref.update_white_balance()
        assert torch.equal(isp.white_balance_gains, ref.white_balance_gains)
    # a grid change rebuilds E from the new grid and the current gains; a grid of another shape gets a new E
    g = isp.white_balance_gains.cpu().numpy()
    for grid in (make_grid(rng, 4, 4, 4), make_grid(rng, 4, 4, 1), make_grid(rng, 8, 3, 4)):
        isp.set(lens_shading=grid)
        assert np.array_equal(isp._awb_E.cpu().numpy(), A.effective(g, 3, grid))
    isp.set(lens_shading=False)
    assert np.array_equal(isp._awb_E.cpu().numpy(), A.effective(g, 3))


def test_graph_capture_of_a_step(ti, rng, dev):
    frames = [[torch.from_numpy(pack(scene_codes(rng, H, W, 0, CASTS[(k + j) % 3], 4095), "std")).to(dev)
               for j in range(2)] for k in range(4)]
    static = [torch.empty_like(f) for f in frames[0]]
    cap = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev, auto_white_balance=True)
    eager = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.5, device=dev, auto_white_balance=True)

    def step(isp, srcs):
        imgs = isp.load_packed12_batch(srcs)
        return imgs, isp.tonemap_reinhard(imgs, write_back=False)

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
        imgs, _ = step(cap, static)
    for k in range(1, 4):
        for s, f in zip(static, frames[k]):
            s.copy_(f)
        g.replay()
        want, _ = step(eager, frames[k])
        torch.cuda.synchronize(dev)
        for a, b in zip(imgs, want):
            assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"replay {k}")
        assert torch.equal(cap.white_balance_gains, eager.white_balance_gains), k
        assert torch.equal(cap._awb_E, eager._awb_E)


def test_gray_world_recovers_the_synthetic_cast(ti, dev):
    from taichi_image_amd import synthetic
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=1.0, device=dev, auto_white_balance=True)
    for k in range(3):
        isp.load_packed12(torch.from_numpy(synthetic.synthetic_packed12(k, 384, 512)).to(dev))
        isp.update_white_balance()
        g = isp.white_balance_gains.cpu().numpy().astype(np.float64)
        assert np.allclose(g, [0.8, 1.0, 4 / 3], rtol=0.02), (k, g)
