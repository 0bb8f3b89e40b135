"""GPU parity off the fast paths: orientation transforms, resizes under a transform, and buffers that are views.

With a transform set, the ISP tonemaps never take their FULL path (csrc/isp_elementwise.hip: `can_full` needs no
transform); every pixel goes through the per-pixel scatter of the general path.  With a buffer that is a view at an
offset, the kernels choose scalar IO from the pointer (`vec_ok`, `vec_store_ok`, `src_fast`, `hot_spec`).  Here both
meet the oracle (oracle/isp_oracle.py) at shapes whose last group of 8 pixels is ragged (34 x 130: H * W = 4 mod 8),
at shapes that span several blocks, and over consecutive steps of a rolling metering; and every result on a view is
also compared bit for bit with the same call on fresh allocations.

Contracts as elsewhere: loads bit-exact, u8 outputs and the in-place p within `assert_close`.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests.util import assert_close, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = ["Camera16", "Camera32"]
WORK = {"Camera16": "f16", "Camera32": "f32"}
TORCH = {"Camera16": torch.float16, "Camera32": torch.float32}
BITS = {"Camera16": torch.int16, "Camera32": torch.int32}
SWAP = ("rotate_90", "rotate_270", "transpose")
# one parameter set per step: gamma 1 (no pow), the colour-adapt variant of the kernels, a non-integral 1/gamma
STEPS = [dict(gamma=0.6, intensity=1.0, light_adapt=1.0, color_adapt=0.0),
         dict(gamma=1.0, intensity=1.2, light_adapt=0.8, color_adapt=0.2),
         dict(gamma=2.2, intensity=0.9, light_adapt=1.0, color_adapt=0.0)]
# (34, 130): H * W = 4 (mod 8) - the last group is ragged and n_px is no multiple of 512; (200, 512): several blocks,
# not square.  transverse is defined for square images only; 66 x 66 and 130 x 130 both end in a ragged group.
TRANSFORM_CASES = ([(name, shape) for name in O.TRANSFORMS if name != "transverse" for shape in [(34, 130), (200, 512)]]
                   + [("transverse", (66, 66)), ("transverse", (130, 130))])


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def dst_shape(H, W, name):
    return (W, H, 3) if name in SWAP else (H, W, 3)


def frames_of(seed, H, W, n=3, step=0):
    """n cameras of differing brightness; the scene darkens a little from step to step (the metering rolls)."""
    return [natural_packed12(np.random.default_rng(seed + 10 * step + k), H, W, dark=0.15 * k + 0.04 * step) for k in range(n)]


# ---- 1. orientation transforms against the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("name,shape", TRANSFORM_CASES)
def test_isp_tonemaps_with_a_transform_against_the_oracle(ti, dev, cam, name, shape):
    """Three steps, moving_alpha 0.1, three cameras: tonemap_reinhard with and without the write-back, tonemap_linear,
    tonemap_reinhard_yuv420, tonemap_only and the static kernels, each against O.transform of the oracle's output."""
    H, W = shape
    work, t = WORK[cam], ti.ImageTransform(name)
    out_shape = dst_shape(H, W, name)

    def make():
        return getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.1, transform=t, device=dev)
    wb, keep, lin, yuv = make(), make(), make(), make()
    st = O.IspState(0.1)
    for step, kw in enumerate(STEPS):
        packs = frames_of(2000, H, W, step=step)
        frames = [torch.from_numpy(p).to(dev) for p in packs]
        refs = [O.isp_load_packed12(p, work) for p in packs]
        ia, ib, ic, id_ = ([isp.load_packed12(f) for f in frames] for isp in (wb, keep, lin, yuv))
        for k in range(3):
            assert_exact(ia[k].cpu().numpy(), refs[k], f"step {step} load {k}")
        before = [im.clone() for im in ib]
        oa = wb.tonemap_reinhard(ia, **kw)
        ob = keep.tonemap_reinhard(ib, write_back=False, **kw)
        oc = lin.tonemap_linear(ic, gamma=kw["gamma"])
        od = yuv.tonemap_reinhard_yuv420(id_, **kw)
        m = st.update_metering(refs)
        for what, isp in (("write_back", wb), ("keep", keep), ("linear", lin), ("yuv", yuv)):
            assert_close(isp.metrics.cpu().numpy(), m, f"step {step} {what}: metrics", rel=2e-5)
        metrics = wb.metrics
        for k in range(3):
            tag = f"{cam} {name} {shape} step {step} camera {k}"
            ref_u8, ref_p = O.reinhard_isp(refs[k], m, **kw)
            want = O.transform(ref_u8, name)
            want_lin = O.transform(O.linear_isp(refs[k], m, kw["gamma"]), name)
            assert want.shape == out_shape
            for what, o in (("write_back", oa[k]), ("keep", ob[k]), ("linear", oc[k])):
                assert tuple(o.shape) == out_shape and o.dtype == torch.uint8, f"{tag} {what}: shape {tuple(o.shape)}"
            assert_close(oa[k].cpu().numpy(), want, f"{tag}: reinhard")
            assert_close(ia[k].cpu().numpy(), ref_p, f"{tag}: in-place p")
            assert_close(ob[k].cpu().numpy(), want, f"{tag}: reinhard write_back=False")
            assert torch.equal(ib[k].view(BITS[cam]), before[k].view(BITS[cam])), f"{tag}: write_back=False changed the image"
            assert_close(oc[k].cpu().numpy(), want_lin, f"{tag}: linear")
            want_yuv = O.rgb_yuv420(want)
            assert tuple(od[k].shape) == want_yuv.shape, f"{tag}: yuv shape {tuple(od[k].shape)}"
            assert_close(od[k].cpu().numpy(), want_yuv, f"{tag}: yuv420")
            assert_close(id_[k].cpu().numpy(), ref_p, f"{tag}: yuv420 in-place p")
            # tonemap_only and the static kernels, on the loaded image (tonemap_linear leaves it as it is), with the ISP's
            # own metrics
            src = ic[k].clone()
            o1 = wb.tonemap_only(src, metrics, kw["gamma"], kw["intensity"], kw["light_adapt"], kw["color_adapt"])
            assert tuple(o1.shape) == out_shape
            assert_close(o1.cpu().numpy(), want, f"{tag}: tonemap_only")
            assert_close(src.cpu().numpy(), ref_p, f"{tag}: tonemap_only in-place p")
            src = ic[k].clone()
            o2 = torch.empty(out_shape, dtype=torch.uint8, device=dev)
            type(wb).reinhard_kernel(src, o2, metrics, kw["gamma"], kw["intensity"], kw["light_adapt"], kw["color_adapt"], t)
            assert_close(o2.cpu().numpy(), want, f"{tag}: reinhard_kernel")
            o3 = torch.empty(out_shape, dtype=torch.uint8, device=dev)
            type(wb).linear_kernel(ic[k], o3, metrics, kw["gamma"], t)
            assert_close(o3.cpu().numpy(), want_lin, f"{tag}: linear_kernel")


@pytest.mark.parametrize("name", ["rotate_90", "transpose"])
@pytest.mark.parametrize("cam,kw,shape,dst", [("Camera16", dict(resize_width=130), (96, 256), (49, 130)),
                                               ("Camera32", dict(scale=0.5), (68, 260), (34, 130))])
def test_isp_resize_with_a_transform(ti, dev, name, cam, kw, shape, dst):
    """A resize and a transform on one camera: the destination (49 x 130, 34 x 130) ends in a ragged group."""
    H, W = shape
    work = WORK[cam]
    a = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.1, transform=ti.ImageTransform(name), device=dev, **kw)
    b = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.1, transform=ti.ImageTransform(name), device=dev, **kw)
    assert (dst[0] * dst[1]) % 8 != 0
    st = O.IspState(0.1)
    for step in range(2):
        packs = frames_of(2100, H, W, step=step)
        frames = [torch.from_numpy(p).to(dev) for p in packs]
        refs = [O.isp_load_packed12(p, work, resize_width=kw.get("resize_width", 0), scale=kw.get("scale")) for p in packs]
        ia, ib = [a.load_packed12(f) for f in frames], [b.load_packed12(f) for f in frames]
        for k in range(3):
            assert ia[k].shape == (*dst, 3)
            assert_exact(ia[k].cpu().numpy(), refs[k], f"step {step} load {k}")
        oa = a.tonemap_reinhard(ia, gamma=0.6)
        ob = b.tonemap_linear(ib, gamma=0.8)
        m = st.update_metering(refs)
        assert_close(a.metrics.cpu().numpy(), m, f"step {step}: metrics", rel=2e-5)
        assert_close(b.metrics.cpu().numpy(), m, f"step {step}: metrics (linear)", rel=2e-5)
        for k in range(3):
            ref_u8, ref_p = O.reinhard_isp(refs[k], m, gamma=0.6)
            assert tuple(oa[k].shape) == dst_shape(*dst, name) == tuple(ob[k].shape)
            assert_close(oa[k].cpu().numpy(), O.transform(ref_u8, name), f"step {step} camera {k}: reinhard")
            assert_close(ia[k].cpu().numpy(), ref_p, f"step {step} camera {k}: in-place p")
            assert_close(ob[k].cpu().numpy(), O.transform(O.linear_isp(refs[k], m, 0.8), name), f"step {step} camera {k}: linear")


def test_isp_process_packed12_with_a_transform_against_the_oracle(ti, dev):
    """process_packed12 on a camera with a transform takes the two calls; against the oracle at a non-square shape with
    a ragged group, two groups of a rolling metering."""
    H, W, n = 34, 130, 3
    isp = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.1, transform=ti.ImageTransform.rotate_270, device=dev)
    st = O.IspState(0.1)
    for group in range(2):
        packs = frames_of(2200, H, W, n, step=group)
        outs, images = isp.process_packed12([torch.from_numpy(p).to(dev) for p in packs], gamma=0.6, keep_images=True)
        refs = [O.isp_load_packed12(p, "f16") for p in packs]
        m = st.update_metering(refs)
        assert_close(isp.metrics.cpu().numpy(), m, f"group {group}: metrics", rel=2e-5)
        for k in range(n):
            ref_u8, ref_p = O.reinhard_isp(refs[k], m, gamma=0.6)
            assert tuple(outs[k].shape) == (W, H, 3)
            assert_close(outs[k].cpu().numpy(), O.transform(ref_u8, "rotate_270"), f"group {group} camera {k}: u8")
            assert_close(images[k].cpu().numpy(), ref_p, f"group {group} camera {k}: p")


def _frame_batch(ti, dev, packs, images, outs, H, W, state, alpha, tonemap, gamma, transform, ws):
    from taichi_image_amd import _native
    L = _native.lib()
    return L.mi_isp_camera_frame_batch(_native.ptr_array(packs), _native.ptr_array(images), _native.ptr_array(outs), len(packs),
                                       H, W, 12, 0, 0, None, ti.types.f16.code, H, W, ctypes.c_float(0.0), 8,
                                       state.data_ptr(), ctypes.c_float(alpha), tonemap, ctypes.c_float(gamma),
                                       ctypes.c_float(1.0), ctypes.c_float(1.0), ctypes.c_float(0.0),
                                       ti.interpolate.transform_code(transform), ws.data_ptr(), _native.stream_ptr(dev))


@pytest.mark.parametrize("name", ["rotate_270", "transpose"])
@pytest.mark.parametrize("tonemap", [0, 1])
def test_camera_frame_batch_with_a_transform_against_the_oracle(ti, dev, name, tonemap):
    """mi_isp_camera_frame_batch straight through ctypes: packed bytes of three cameras -> transformed u8 outputs in one
    call, two groups, against the oracle (not against the Python ISP)."""
    from taichi_image_amd import _native
    L = _native.lib()
    H, W, n = 34, 130, 3
    state = torch.zeros(9, dtype=torch.float32, device=dev)
    images = [torch.empty((H, W, 3), dtype=torch.float16, device=dev) for _ in range(n)]
    outs = [torch.empty(dst_shape(H, W, name), dtype=torch.uint8, device=dev) for _ in range(n)]
    ws = torch.zeros(int(L.mi_isp_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    st = O.IspState(0.25)
    for group in range(2):
        packs = frames_of(2300, H, W, n, step=group)
        rc = _frame_batch(ti, dev, [torch.from_numpy(p).to(dev) for p in packs], images, outs, H, W, state,
                          0.0 if group == 0 else 0.75, tonemap, 0.6, ti.ImageTransform(name), ws)
        assert rc == 0, L.mi_isp_last_error()
        refs = [O.isp_load_packed12(p, "f16") for p in packs]
        m = st.update_metering(refs)
        assert_close(state.cpu().numpy(), m, f"group {group}: state", rel=2e-5)
        for k in range(n):
            if tonemap == 0:
                ref_u8, ref_img = O.reinhard_isp(refs[k], m, gamma=0.6)
            else:
                ref_u8, ref_img = O.linear_isp(refs[k], m, 0.6), refs[k]
            assert_close(outs[k].cpu().numpy(), O.transform(ref_u8, name), f"group {group} camera {k}: u8")
            assert_close(images[k].cpu().numpy(), ref_img, f"group {group} camera {k}: image left behind")


# ---- 2. the two fixes ----------------------------------------------------------------------------------------------------
def test_transverse_on_a_non_square_image_leaves_the_state_alone(ti, dev):
    """transverse takes square images only.  The ISP tonemaps reject a non-square image before they meter it: the
    metrics and the images are as they were after the AssertionError.  The C entry does the same for state9."""
    from taichi_image_amd import _native
    L = _native.lib()
    isp = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.3, transform=ti.ImageTransform.transverse, device=dev)
    sq = [isp.load_packed12(torch.from_numpy(p).to(dev)) for p in frames_of(2400, 66, 66, 2)]
    isp.tonemap_reinhard(sq, gamma=0.6)
    images = [isp.load_packed12(torch.from_numpy(p).to(dev)) for p in frames_of(2410, 34, 130, 2)]
    before = [im.clone() for im in images]
    for call in (lambda: isp.tonemap_reinhard(images, gamma=0.6), lambda: isp.tonemap_reinhard(images, write_back=False),
                 lambda: isp.tonemap_linear(images, gamma=0.8), lambda: isp.tonemap_reinhard_yuv420(images, gamma=0.6),
                 lambda: isp.process_packed12([torch.from_numpy(p).to(dev) for p in frames_of(2410, 34, 130, 2)])):
        old, snap = isp.metrics, isp.metrics.clone()
        with pytest.raises(AssertionError):
            call()
        torch.cuda.synchronize()
        assert isp.metrics is old and torch.equal(old, snap), "a call that failed moved the metering state"
        for im, b in zip(images, before):
            assert torch.equal(im.view(torch.int16), b.view(torch.int16)), "a call that failed changed an image"
    fresh = ti.Camera16(ti.BayerPattern.RGGB, transform=ti.ImageTransform.transverse, device=dev)
    with pytest.raises(AssertionError):
        fresh.tonemap_reinhard(images)
    assert fresh.metrics is None
    # the C ABI: rejected before the load and the metering
    H, W = 34, 130
    state = torch.arange(9, dtype=torch.float32, device=dev) * 0.1
    snap = state.clone()
    imgs = [torch.empty((H, W, 3), dtype=torch.float16, device=dev)]
    outs = [torch.empty((H, W, 3), dtype=torch.uint8, device=dev)]
    ws = torch.zeros(int(L.mi_isp_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    rc = _frame_batch(ti, dev, [torch.from_numpy(frames_of(2420, H, W, 1)[0]).to(dev)], imgs, outs, H, W, state, 0.7, 0,
                      0.6, ti.ImageTransform.transverse, ws)
    torch.cuda.synchronize()
    assert rc != 0 and b"transverse" in L.mi_isp_last_error()
    assert torch.equal(state, snap), "mi_isp_camera_frame_batch moved state9 before it rejected the transform"


def _at_byte_offset(packed, offset, dev):
    """A packed frame as a view `offset` bytes into a device buffer (contiguous, so the library takes it as it is)."""
    n = packed.size
    buf = torch.zeros(offset + n + 64, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + n].view(packed.shape)
    view.copy_(torch.from_numpy(packed))
    assert view.is_contiguous() and view.data_ptr() % 16 == offset % 16
    return view


def test_isp_process_packed12_on_a_frame_at_a_byte_offset(ti, dev):
    """A frame 2 bytes off a 4-byte boundary is a legal input of load_packed12_batch; process_packed12 on a group with one
    such frame gives what load_packed12_batch + tonemap_reinhard give (outputs, images, metrics), over two groups."""
    H, W, n = 48, 512, 3
    from taichi_image_amd import _native
    assert _native.lib().mi_isp_camera_group_fits(H, W, 0, ti.types.f16.code, 8) == 1
    a = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    b = ti.Camera16(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    st = O.IspState(0.3)
    for group in range(2):
        packs = frames_of(2500, H, W, n, step=group)
        frames = [torch.from_numpy(p).to(dev) for p in packs]
        frames[1] = _at_byte_offset(packs[1], 2, dev)
        outs, images = a.process_packed12(frames, gamma=0.6, keep_images=True)
        want_images = b.load_packed12_batch(frames)
        want = b.tonemap_reinhard(want_images, gamma=0.6)
        assert torch.equal(a.metrics.view(torch.int32), b.metrics.view(torch.int32)), f"group {group}: metrics"
        m = st.update_metering([O.isp_load_packed12(p, "f16") for p in packs])
        assert_close(a.metrics.cpu().numpy(), m, f"group {group}: metrics against the oracle", rel=2e-5)
        for k in range(n):
            assert torch.equal(outs[k], want[k]), f"group {group} camera {k}: u8"
            assert torch.equal(images[k].view(torch.int16), want_images[k].view(torch.int16)), f"group {group} camera {k}: p"


# ---- 3. view-backed buffers ---------------------------------------------------------------------------------------------
def _stacked_views(cam, n, H, W, dev):
    """n (H, W, 3) images that are views into one buffer, and the sentinel region behind them.  Camera16: the slices of
    an (n + 1, H, W, 3) stack - with H * W = 4 (mod 8) every odd one sits 8 bytes off 16.  An f32 stack stays aligned, so
    Camera32 reaches the scalar paths through a one-element storage offset: every image sits 4 bytes off 16."""
    dt = TORCH[cam]
    if cam == "Camera16":
        buf = torch.empty((n + 1, H, W, 3), dtype=dt, device=dev)
        views, guard = list(buf.unbind(0))[:n], [buf[n]]
    else:
        px = H * W * 3
        flat = torch.empty(1 + (n + 1) * px, dtype=dt, device=dev)
        views = [flat[1 + k * px:1 + (k + 1) * px].view(H, W, 3) for k in range(n)]
        guard = [flat[:1], flat[1 + n * px:]]
    for g in guard:
        g.fill_(-1234.0)
    assert all(v.is_contiguous() for v in views)
    assert any(v.data_ptr() % 16 for v in views), "no view is off its 16-byte boundary"
    return views, guard


@pytest.mark.parametrize("cam", CAMS)
def test_isp_on_images_that_are_views(ti, dev, cam):
    """update_metering, tonemap_reinhard (both write_back values), tonemap_linear and tonemap_reinhard_yuv420 (its fallback
    shape) on images that are views at unaligned offsets: against the oracle, bit for bit against the same calls on fresh
    allocations, and nothing written outside the images."""
    H, W, n = 34, 130, 3
    work, bits = WORK[cam], BITS[cam]
    views, guard = _stacked_views(cam, n, H, W, dev)
    guard0 = [g.clone() for g in guard]
    packs = frames_of(2600, H, W, n)
    refs = [O.isp_load_packed12(p, work) for p in packs]
    srcs = [torch.from_numpy(r).to(dev) for r in refs]
    a = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    b = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=0.3, device=dev)
    st = O.IspState(0.3)

    def fill():
        for v, s in zip(views, srcs):
            v.copy_(s)
        return [s.clone() for s in srcs]

    calls = [("update_metering", lambda isp, ims: isp.update_metering(ims)),
             ("reinhard", lambda isp, ims: isp.tonemap_reinhard(ims, gamma=0.6, color_adapt=0.2)),
             ("reinhard keep", lambda isp, ims: isp.tonemap_reinhard(ims, gamma=0.6, write_back=False)),
             ("linear", lambda isp, ims: isp.tonemap_linear(ims, gamma=0.8)),
             ("yuv420", lambda isp, ims: isp.tonemap_reinhard_yuv420(ims, gamma=0.6))]
    for what, call in calls:
        fresh = fill()
        got, want = call(a, views), call(b, fresh)
        torch.cuda.synchronize()
        m = st.update_metering(refs)
        assert torch.equal(a.metrics.view(torch.int32), b.metrics.view(torch.int32)), f"{what}: metrics"
        assert_close(a.metrics.cpu().numpy(), m, f"{what}: metrics", rel=2e-5)
        for g, g0 in zip(guard, guard0):
            assert torch.equal(g, g0), f"{what}: wrote outside the images"
        for k in range(n):
            assert torch.equal(views[k].view(bits), fresh[k].view(bits)), f"{what} image {k}: left behind differs"
        if got is None:
            continue
        kw = dict(gamma=0.6, color_adapt=0.2) if what == "reinhard" else dict(gamma=0.6)
        for k in range(n):
            assert torch.equal(got[k], want[k]), f"{what} image {k}: output differs from fresh allocations"
            if what == "linear":
                assert_close(got[k].cpu().numpy(), O.linear_isp(refs[k], m, 0.8), f"{what} image {k}")
                assert_exact(views[k].cpu().numpy(), refs[k], f"{what} image {k}: image changed")
                continue
            ref_u8, ref_p = O.reinhard_isp(refs[k], m, **kw)
            assert_close(got[k].cpu().numpy(), O.rgb_yuv420(ref_u8) if what == "yuv420" else ref_u8, f"{what} image {k}")
            if what == "reinhard keep":
                assert_exact(views[k].cpu().numpy(), refs[k], f"{what} image {k}: image changed")
            else:
                assert_close(views[k].cpu().numpy(), ref_p, f"{what} image {k}: in-place p")


def _offset_view(arr, dev):
    """`arr` on the device at a one-element storage offset."""
    arr = np.ascontiguousarray(arr)
    e = arr.itemsize
    flat = torch.zeros(e + arr.nbytes, dtype=torch.uint8, device=dev)     # (byte copies: no op of the element type needed)
    flat[e:].copy_(torch.from_numpy(arr.reshape(-1).view(np.uint8)))
    v = flat[e:].view(torch.from_numpy(arr[:0].reshape(-1)).dtype).view(arr.shape)
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 != 0
    return v


def _rgb(seed, H, W, dt):
    img = O.bayer_to_rgb(O.decode12(natural_packed12(np.random.default_rng(seed), H, W), "f32", scaled=True))
    return (np.clip(img, 0, 1) * 255).astype(np.uint8) if dt == "u8" else img.astype(O.NP_DTYPE[dt])


@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_stateless_calls_on_a_one_element_offset(ti, dev, dt):
    """tonemap_linear, tonemap_reinhard, resize_bilinear, transform, rgb_yuv420 and bayer_to_rgb on inputs that sit one
    element past the start of their storage: against the oracle, and equal to the same call on an aligned copy."""
    from taichi_image_amd import color
    img = _rgb(2700, 34, 130, dt)
    v, aligned = _offset_view(img, dev), torch.from_numpy(img).to(dev)
    for what, fn, want, exact in (
            ("tonemap_linear", lambda x: ti.tonemap.tonemap_linear(x, gamma=0.8), O.tonemap_linear(img, 0.8, "u8"), False),
            ("tonemap_reinhard", lambda x: ti.tonemap.tonemap_reinhard(x, gamma=0.6, color_adapt=0.2),
             O.tonemap_reinhard(img, gamma=0.6, color_adapt=0.2), False),
            ("tonemap_reinhard f16", lambda x: ti.tonemap.tonemap_reinhard(x, dtype=ti.types.f16),
             O.tonemap_reinhard(img, dtype="f16"), False),
            ("resize_bilinear", lambda x: ti.interpolate.resize_bilinear(x, (104, 27), 0.8),
             O.resize_bilinear(img, (104, 27), 0.8), True),
            ("rgb_yuv420", lambda x: color.rgb_yuv420_image(x, dtype=ti.types.u8), O.rgb_yuv420(img, "u8"), False)):
        got = fn(v)
        assert_exact(got.cpu().numpy(), fn(aligned).cpu().numpy(), f"{what} {dt}: offset view against an aligned copy")
        (assert_exact if exact else assert_close)(got.cpu().numpy(), want, f"{what} {dt}")
    for name in O.TRANSFORMS:
        src = _rgb(2710, 34, 34, dt) if name == "transverse" else img
        got = ti.interpolate.transform(_offset_view(src, dev), ti.ImageTransform(name))
        assert_exact(got.cpu().numpy(), O.transform(src, name), f"transform {name} {dt}")
    cfa = O.decode12(natural_packed12(np.random.default_rng(2720), 34, 130), "u16" if dt == "u8" else dt, scaled=dt != "u8")
    for p in range(4):
        got = ti.bayer.bayer_to_rgb(_offset_view(cfa, dev), ti.BayerPattern(p))
        assert_exact(got.cpu().numpy(), O.bayer_to_rgb(cfa, p), f"bayer_to_rgb pattern {p} {cfa.dtype}")


@pytest.mark.parametrize("offset", [1, 2, 3, 4])
def test_packed_frames_at_byte_offsets(ti, dev, offset):
    """Packed frames `offset` bytes into a device buffer, W % 8 == 0 (so only the pointer turns the fast source path
    off, for offsets 1 - 3): load_packed12 with no resize, with a resize and on Camera32, load_packed12_batch over aligned
    and offset frames mixed, pipeline12_reinhard - bit-exact against the oracle and against aligned copies."""
    from taichi_image_amd.pipeline import pipeline12_reinhard
    H, W = 34, 136
    packs = frames_of(2800, H, W, 3)
    for cam, kw in (("Camera16", {}), ("Camera16", dict(resize_width=90)), ("Camera32", {})):
        isp = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, **kw)
        refs = [O.isp_load_packed12(p, WORK[cam], resize_width=kw.get("resize_width", 0)) for p in packs]
        aligned = [torch.from_numpy(p).to(dev) for p in packs]
        views = [_at_byte_offset(p, offset, dev) for p in packs]
        got = isp.load_packed12(views[0])
        assert_exact(got.cpu().numpy(), refs[0], f"{cam} {kw} load_packed12 at +{offset}")
        assert torch.equal(got, isp.load_packed12(aligned[0])), f"{cam} {kw}: offset frame differs from an aligned copy"
        mixed = [aligned[0], views[1], aligned[2]] if offset != 4 else views
        batch = isp.load_packed12_batch(mixed)
        for k in range(3):
            assert_exact(batch[k].cpu().numpy(), refs[k], f"{cam} {kw} load_packed12_batch frame {k} at +{offset}")
    want = O.pipeline12_reinhard(packs[0])
    got = pipeline12_reinhard(views[0], whole_frame=False)
    assert torch.equal(got.view(torch.int16), pipeline12_reinhard(aligned[0], whole_frame=False).view(torch.int16)), \
        f"pipeline12 at +{offset}: offset frame differs from an aligned copy"
    assert_close(got.cpu().numpy(), want, f"pipeline12 at +{offset}")
    # the default call picks the whole-frame kernel for the frames it takes; a frame off its 4-byte boundary is not one
    assert_close(pipeline12_reinhard(views[0]).cpu().numpy(), want, f"pipeline12 default chain at +{offset}")
