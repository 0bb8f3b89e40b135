"""Local tone mapping on the GPU ("Local tone mapping"): the bilateral grid (all four planes) and the mapped
image against tests/local_tonemap_ref.py bit for bit, through the C ABI and through Camera16 / Camera32; every loader
family with the stage on against the same loader with it off followed by local_tonemap(); process_packed12; the stage off;
the error paths."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import exposure_merge_ref as EM
from tests import local_tonemap_ref as R
from tests.test_gpu_denoise import call
from tests.test_gpu_exposure_merge import GAIN, RATIOS, READ_NOISE, load as load_bracket
from tests.test_gpu_temporal import encode
from tests.util import _count_calls, assert_exact, natural_packed12

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
CCM = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]
ENTRIES = ["mi_isp_local_tonemap_workspace_bytes", "mi_isp_local_tonemap_batch", "mi_isp_local_tonemap_grids"]
INPUTS = R.gpu_test_inputs()
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def reference(i):
    """(grids, mapped image) of input i by the reference: computed once, never written."""
    _, img, kw = INPUTS[i]
    return R.grids(img, kw), R.local_tonemap(img, kw)


def settings(ti, kw):
    return ti.LocalTonemap(**kw)


def mapped(ti, images, s):
    """The off-loader images through local_tonemap()."""
    return ti.local_tonemap.local_tonemap(images, s)


# ---- the C ABI: grids() and local_tonemap() ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(INPUTS)), ids=[n for n, _, _ in INPUTS])
def test_grids_and_image_against_the_reference(ti, dev, i):
    name, img, kw = INPUTS[i]
    s = settings(ti, kw)
    (cnt, sm, nb, sb), want = reference(i)
    t = torch.from_numpy(img).to(dev)
    got = ti.local_tonemap.grids(t, s)
    assert all(g.device == dev and tuple(g.shape) == cnt.shape for g in got)
    assert_exact(got[0].cpu().numpy().view(np.uint32), cnt, name + " cnt")
    assert_exact(got[1].cpu().numpy().view(np.uint32), sm, name + " sum")
    assert_exact(got[2].cpu().numpy(), nb, name + " Nb")
    assert_exact(got[3].cpu().numpy(), sb, name + " Sb")
    out = mapped(ti, t, s)
    assert out.device == dev and out.data_ptr() != t.data_ptr()
    assert_exact(t.cpu().numpy(), img, name + " the input (left as it was)")
    assert_exact(out.cpu().numpy(), want, name + " image")
    if i % 6 == 0:                                                 # numpy in, numpy out
        host = mapped(ti, img, s)
        assert isinstance(host, np.ndarray)
        assert_exact(host, want, name + " image (numpy)")
        hg = ti.local_tonemap.grids(img, s)
        assert hg[0].dtype == np.uint32
        assert_exact(hg[0], cnt, name + " cnt (numpy)")
        assert_exact(hg[3], sb, name + " Sb (numpy)")


@pytest.mark.parametrize("work", ["f16", "f32"])
def test_properties_on_the_device(ti, rng, dev, work):
    """strength == 0 returns the image bit for bit; the three channels share one gain, which is >= 1 for anchor == white."""
    dtype = np.float16 if work == "f16" else np.float32
    img = R.make_image(rng, 66, 70, "wide", dtype)
    assert_exact(mapped(ti, img, ti.LocalTonemap(0.0, cell=16)), img, "strength 0")
    pos = np.abs(img)
    out = mapped(ti, pos.astype(f32), ti.LocalTonemap(0.7, cell=8, bins=8))
    g = R.gain(pos.astype(f32), dict(strength=0.7, cell=8, bins=8))
    assert g.min() >= 1.0
    assert_exact(out, (pos.astype(f32) * g[..., None]).astype(f32), "one gain per pixel")


@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("work", ["f16", "f32"])
def test_batches_with_different_content(ti, dev, monkeypatch, n, work):
    """n images of one geometry in ONE call: each equals the reference of its own content."""
    dtype = np.float16 if work == "f16" else np.float32
    H, W, kw = (66, 70, dict(cell=16, bins=8)) if work == "f16" else (24, 40, dict(cell=8, bins=32, strength=0.8))
    imgs = [R.make_image(np.random.default_rng(50 + k), H, W, R.CONTENTS[k % 3], dtype) for k in range(n)]
    ts = [torch.from_numpy(im).to(dev) for im in imgs]
    calls = _count_calls(monkeypatch, "mi_isp_local_tonemap_batch")
    outs = mapped(ti, ts, settings(ti, kw))
    assert len(calls) == 1 and len(outs) == n
    for k, (o, im) in enumerate(zip(outs, imgs)):
        assert_exact(o.cpu().numpy(), R.local_tonemap(im, kw), f"{work} image {k} of {n}")


# ---- the cameras -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("k", range(len(R.SHAPE_SETTINGS)))
def test_cameras_against_the_reference(ti, rng, dev, cam, work, k):
    """load_packed12 with the stage on = the reference on the image of the same loader without it."""
    H, W, kw = R.SHAPE_SETTINGS[k]
    src = torch.from_numpy(natural_packed12(rng, H, W)).to(dev)
    args = dict(device=dev, correct_colors=True, color_correction=CCM)
    off = getattr(ti, cam)(ti.BayerPattern.RGGB, **args).load_packed12(src).cpu().numpy()
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, local_tonemap=settings(ti, kw), **args)
    assert isp.local_tonemap == settings(ti, kw)
    got = isp.load_packed12(src)
    assert_exact(got.cpu().numpy(), R.local_tonemap(off, kw), f"{cam} {H}x{W} {kw}")


def make_source(rng, kind, H, W):
    u = np.clip(0.02 + 0.9 * rng.random((H, W)) ** 3, 0, 1)
    return torch.from_numpy(np.ascontiguousarray(encode(kind, u)[0]))


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_single_frame_loaders(ti, rng, dev, monkeypatch, cam, work, kind):
    """The five single-frame loaders (and the IDS packing): the stage on = the loader without it, then local_tonemap();
    one call of the library, behind the resize, the lens remap and the defect fix-up; no metering subsample."""
    H, W = 66, 72
    s = ti.LocalTonemap(0.6, cell=16, bins=8, white=1000.0 if kind == "16f" else 1.0, floor=1.0 if kind == "16f" else 2.0 ** -10)
    src = make_source(rng, kind, H, W).to(dev)
    dm = ti.DefectMap([[3, 4], [20, 61], [41, 70], [65, 71]], (H, W))
    K = np.array([[100.0, 0, W / 2], [0, 100.0, H / 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, [-0.1, 0.02, 0.001, -0.001], (H, W))
    for extra, kw in ((dict(), dict()), (dict(resize_width=48), dict(defects=dm)), (dict(), dict(defects=dm, undistort=lens)),
                      (dict(raw_denoise=ti.RawDenoise(2.4e-4, 1.5e-3)), dict())):
        args = dict(device=dev, correct_colors=True, **extra)
        off = getattr(ti, cam)(ti.BayerPattern.GRBG, **args)
        on = getattr(ti, cam)(ti.BayerPattern.GRBG, local_tonemap=s, **args)
        want = mapped(ti, call(off, kind, src, **kw), s)
        calls = [_count_calls(monkeypatch, e) for e in ENTRIES]
        got = call(on, kind, src, **kw)
        assert [len(c) for c in calls][1:] == [1, 0]
        monkeypatch.undo()
        assert not hasattr(got, "_mi_metering_sub")
        assert_exact(got.cpu().numpy(), want.cpu().numpy(), f"{cam} {kind} {extra} {list(kw)}")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("bits", [12, 16])
def test_batch_loaders(ti, rng, dev, monkeypatch, cam, work, bits):
    """The two batch loaders: one call of the stage for all images of the batch."""
    H, W, n = 66, 72, 3
    s = ti.LocalTonemap(0.5, cell=32, bins=16)
    kind = "p12" if bits == 12 else "p16"
    srcs = [make_source(rng, kind, H, W).to(dev) for _ in range(n)]
    for extra in (dict(), dict(resize_width=40)):
        off = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, **extra)
        on = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, local_tonemap=s, **extra)
        name = f"load_packed{bits}_batch"
        want = mapped(ti, getattr(off, name)(srcs), s)
        calls = _count_calls(monkeypatch, "mi_isp_local_tonemap_batch")
        got = getattr(on, name)(srcs)
        assert len(calls) == 1
        monkeypatch.undo()
        for k in range(n):
            assert not hasattr(got[k], "_mi_metering_sub")
            assert_exact(got[k].cpu().numpy(), want[k].cpu().numpy(), f"{cam} {name} {extra} image {k}")
        assert getattr(on, name)([]) == []


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "p16", "16u", "16f", "32f", "p12_batch", "p16_batch"])
def test_bracket_loaders(ti, rng, dev, monkeypatch, cam, work, kind):
    """All seven bracket loaders behind the exposure merge."""
    H, W, E = 66, 72, 2
    base = kind.split("_")[0]
    scale = 1000.0 if base == "16f" else 1.0
    s = ti.LocalTonemap(0.5, cell=16, bins=16, white=scale, floor=scale * 2.0 ** -10)
    em = ti.ExposureMerge(RATIOS[E], GAIN * scale, READ_NOISE * scale, saturation=0.9 * scale)
    n = 2 if kind.endswith("_batch") else 1
    brackets = [[torch.from_numpy(np.ascontiguousarray(encode(base, u)[0])).to(dev)
                 for u in EM.make_bracket(rng, H, W, RATIOS[E], GAIN, READ_NOISE)] for _ in range(n)]
    off = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, exposure_merge=em)
    on = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, exposure_merge=em, local_tonemap=s)

    def run(isp):
        if kind == "p12_batch":
            return isp.load_packed12_bracket_batch(brackets)
        if kind == "p16_batch":
            return isp.load_packed16_bracket_batch(brackets)
        return [load_bracket(isp, base, brackets[0])]

    want = mapped(ti, run(off), s)
    calls = _count_calls(monkeypatch, "mi_isp_local_tonemap_batch")
    got = run(on)
    assert len(calls) == 1
    for k in range(n):
        assert_exact(got[k].cpu().numpy(), want[k].cpu().numpy(), f"{cam} {kind} bracket {k}")


@pytest.mark.parametrize("cam,work", CAMS)
def test_the_tonemaps_see_the_mapped_image_and_process_packed12_is_the_two_calls(ti, rng, dev, cam, work):
    H, W, n = 66, 72, 3
    s = ti.LocalTonemap(0.5, cell=16, bins=16)
    frames = [torch.from_numpy(natural_packed12(rng, H, W)).to(dev) for _ in range(n)]
    one = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, local_tonemap=s)
    two = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, local_tonemap=s)
    off = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3)
    for step in range(2):
        outs, imgs = one.process_packed12(frames, gamma=0.6, keep_images=True)
        loaded = two.load_packed12_batch(frames)
        by_hand = mapped(ti, off.load_packed12_batch(frames), s)
        for a, b in zip(loaded, by_hand):
            assert_exact(a.cpu().numpy(), b.cpu().numpy(), f"step {step} loaded image")
        want = two.tonemap_reinhard(loaded, gamma=0.6)
        ref = off.tonemap_reinhard(by_hand, gamma=0.6)             # (metering and tonemap of the mapped image)
        for k in range(n):
            assert_exact(outs[k].cpu().numpy(), want[k].cpu().numpy(), f"step {step} output {k}")
            assert_exact(outs[k].cpu().numpy(), ref[k].cpu().numpy(), f"step {step} output {k} by hand")
            assert_exact(imgs[k].cpu().numpy(), loaded[k].cpu().numpy(), f"step {step} image {k}")
        assert_exact(one.metrics.cpu().numpy(), two.metrics.cpu().numpy(), "metrics")
        assert_exact(one.metrics.cpu().numpy(), off.metrics.cpu().numpy(), "metrics by hand")


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_off_calls_no_new_entry_point(ti, rng, dev, monkeypatch, cam, work, kind):
    """An ISP without the stage, and one after set(local_tonemap=False), reach no mi_isp_local_tonemap_* entry point and
    give the same bits; set(local_tonemap=None) leaves the stage."""
    H, W = 66, 72
    src = make_source(rng, kind, H, W).to(dev)
    calls = [_count_calls(monkeypatch, e) for e in ENTRIES]
    off = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev)
    s = ti.LocalTonemap(0.5, cell=8)
    on = getattr(ti, cam)(ti.BayerPattern.GBRG, device=dev, local_tonemap=s)
    a = call(off, kind, src)
    assert off.local_tonemap is None and sum(len(c) for c in calls) == 0
    on.set(local_tonemap=None, moving_alpha=0.2)
    assert on.local_tonemap is s
    call(on, kind, src)
    assert len(calls[1]) == 1 and len(calls[2]) == 0
    on.set(local_tonemap=False)
    assert on.local_tonemap is None
    for c in calls:
        c.clear()
    b = call(on, kind, src)
    assert sum(len(c) for c in calls) == 0
    assert_exact(b.cpu().numpy(), a.cpu().numpy(), f"{cam} {kind} off again")
    if kind == "p12":
        assert hasattr(b, "_mi_metering_sub") == hasattr(a, "_mi_metering_sub")
        off.process_packed12([src])
        assert sum(len(c) for c in calls) == 0
    on.set(local_tonemap=ti.LocalTonemap(0.25, cell=64, bins=4))
    assert on.local_tonemap.cell == 64


def test_a_loader_captured_into_a_graph(ti, rng, dev):
    """The stage has no state and makes no host synchronisation: a captured loader replays to the same image."""
    H, W = 66, 72
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, local_tonemap=ti.LocalTonemap(0.5, cell=16))
    src = torch.from_numpy(natural_packed12(rng, H, W)).to(dev)
    ref = isp.load_packed12(src).clone()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        img = isp.load_packed12(src)
    img.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert_exact(img.cpu().numpy(), ref.cpu().numpy(), "the replayed load")


# ---- error paths ---------------------------------------------------------------------------------------------------------------
def test_error_paths(ti, dev):
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = 16, 24
    img = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    good = ti.LocalTonemap()._arg()
    ws = torch.empty(int(L.mi_isp_local_tonemap_workspace_bytes(1, H, W, good)) + 16, dtype=torch.uint8, device=dev)
    assert ws.numel() > 16
    planes = [torch.zeros(16, dtype=torch.float32, device=dev) for _ in range(4)]
    stream = _native.stream_ptr(dev)
    ptrs = _native.ptr_array([img])

    def batch(arg=good, p=ptrs, n=1, h=H, w=W, code=_native.MI_F32, w_ptr=None):
        return L.mi_isp_local_tonemap_batch(p, n, h, w, code, arg, ws.data_ptr() if w_ptr is None else w_ptr, stream)

    def bad(**kw):
        a = ti.LocalTonemap()._arg()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for arg in (bad(strength=-0.5), bad(strength=2.0), bad(strength=float("nan")), bad(white=0.0), bad(white=float("inf")),
                bad(floor=0.0), bad(floor=1e-40), bad(floor=1.0), bad(white=1e30), bad(floor=1.0 - 2.0 ** -24),
                bad(anchor=2.0), bad(anchor=1e-6), bad(anchor=float("nan")), bad(cell=12), bad(cell=0), bad(bins=1),
                bad(bins=33), None):
        assert batch(arg=arg) != 0
        assert "local_tonemap" in L.mi_isp_last_error().decode()
        assert L.mi_isp_local_tonemap_grids(img.data_ptr(), H, W, _native.MI_F32, arg, *[p.data_ptr() for p in planes],
                                            stream) != 0
        assert "local_tonemap" in L.mi_isp_last_error().decode()
        assert L.mi_isp_local_tonemap_workspace_bytes(1, H, W, arg) == 0
    null = (ctypes.c_void_p * 1)(None)
    odd = (ctypes.c_void_p * 1)(img.data_ptr() + 2)
    for kw in (dict(n=-1), dict(h=-1), dict(w=32769), dict(code=_native.MI_U8), dict(code=_native.MI_U16), dict(p=None),
               dict(p=null), dict(p=odd), dict(w_ptr=0), dict(w_ptr=ws.data_ptr() + 4)):
        assert batch(**kw) != 0, kw
        assert "local_tonemap" in L.mi_isp_last_error().decode(), kw
    pp = [p.data_ptr() for p in planes]
    for a in ((None, H, W, _native.MI_F32, good, *pp), (img.data_ptr(), H, W, _native.MI_F32, good, pp[0], None, pp[2], pp[3]),
              (img.data_ptr(), H, W, _native.MI_F32, good, pp[0], pp[0], pp[2], pp[3]),
              (img.data_ptr(), H, W, _native.MI_F32, good, pp[0], pp[1], pp[2] + 2, pp[3]),
              (img.data_ptr(), H, W, 7, good, *pp)):
        assert L.mi_isp_local_tonemap_grids(*a, stream) != 0
        assert "local_tonemap" in L.mi_isp_last_error().decode()
    # successful no-ops: no image, an empty image
    assert batch(n=0, p=None) == 0 and batch(h=0) == 0 and batch(w=0, p=None, w_ptr=0) == 0
    assert L.mi_isp_local_tonemap_workspace_bytes(0, H, W, good) == 0
    empty = np.zeros((0, 5, 3), np.float16)
    assert ti.local_tonemap.local_tonemap(empty, ti.LocalTonemap()).shape == (0, 5, 3)
    assert ti.local_tonemap.local_tonemap([], ti.LocalTonemap()) == []
    torch.cuda.synchronize(dev)
    assert float(img.abs().max()) == 0.0                           # (nothing ran on the refused calls)
    # the Python surface
    with pytest.raises(ValueError, match="share a shape"):
        ti.local_tonemap.local_tonemap([np.zeros((4, 4, 3), f32), np.zeros((4, 6, 3), f32)], ti.LocalTonemap())
    with pytest.raises(ValueError, match="local_tonemap"):
        ti.Camera16(ti.BayerPattern.RGGB, device=dev, local_tonemap=0.5)
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev)
    with pytest.raises(ValueError, match="local_tonemap"):
        isp.set(local_tonemap=True)
    assert isp.local_tonemap is None
