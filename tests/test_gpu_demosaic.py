"""The directional demosaic (Camera16/32 demosaic=, demosaic.directional, the three C entry points) on the GPU against
tests/demosaic_ref.py, bit for bit.

The kernel's tile is 32 x 64 with a halo of 4 before and 8 after: R.SHAPES are the degenerate frames (the mirror folds more
than once), one tile, one tile + 2 and two tiles + 2 each way, so every seam and a ragged last tile are hit.  The frames
are R.stripes_codes, which keep both decisions and both estimates busy (the coverage condition, asserted on the reference
alone, here for the frames with levels and gains and in tests/test_demosaic_cpu.py for the plain ones)."""
import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import demosaic_ref as R
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_denoise import call, capture, loader_x
from tests.test_gpu_shading import PER_SITE, make_grid, pixel_gains
from tests.util import _count_calls, assert_exact

pytestmark = pytest.mark.gpu

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
CCM = np.array([[1.6, -0.3, -0.3], [-0.2, 1.5, -0.3], [-0.1, -0.4, 1.5]])
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]
OUTS = ["u8", "u16", "f16", "f32"]
f32 = np.float32


@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def planes():
    """R.planes of a CFA, computed once per (frame, pattern) and shared: {key: (H, W, 3) f32}, never written."""
    cache = {}

    def get(cfa, pattern):
        key = (cfa.shape, str(cfa.dtype), cfa.tobytes(), pattern)
        if key not in cache:
            cache[key] = R.planes(cfa, pattern)
            cache[key].setflags(write=False)
        return cache[key]
    return get


def source(kind, shape, seed, levels=False):
    """(the loader's input, x as the loader computes it, black, white, the matrix that brings the image into [0, 1])."""
    codes = R.stripes_codes(shape, seed)
    H, W = shape
    lv = levels and kind in ("p12", "ids", "p16", "16u")
    full = 4095 if kind in ("p12", "ids") else 65535
    black, white = (PER_SITE, full - 195) if lv else (None, None)
    ccm = CCM
    if kind in ("p12", "ids"):
        src = O.encode12(codes, ids_format=kind == "ids")
        codes = O.decode12(src, "u16", ids_format=kind == "ids")              # (the IDS packing does not round-trip)
    elif kind == "p16":
        codes = (codes * 16).astype(np.uint16)
        src = codes.view(np.uint8).reshape(H, 2 * W)
    elif kind == "16u":
        src = codes = (codes * 16).astype(np.uint16)
    elif kind == "16f":
        src, ccm = codes, CCM / 4096.0                                         # (load_16f: x = f32(code), up to 4095)
    else:
        src = codes = codes.astype(f32) * f32(1 / 4095)
    return src, loader_x(kind, codes, black, white), black, white, ccm


def route_cfa(x, grid, work):
    """The loaders' CFA: cast_work(x * g)."""
    H, W = x.shape
    return O.cast_out(x if grid is None else (x * pixel_gains(grid, H, W)).astype(f32), work)


RAW = {"p12": (0, 0), "ids": (0, 1), "p16": (1, 0), "16u": (2, 0), "32f": (3, 0), "16f": (4, 0)}   # (MI_RAW_*, ids_format)


def raw_call(name, srcs, outs, shape, kind, work, pattern, black, white, grid, ccm, dev):
    """mi_isp_demosaic_directional_raw_batch / mi_isp_raw_cfa_batch on device tensors."""
    from taichi_image_amd import _native
    H, W = shape
    code = {"f16": _native.MI_F16, "f32": _native.MI_F32}[work]
    lv = _native.levels_arg(black, white)
    g = None if grid is None else torch.from_numpy(grid if grid.ndim == 3 else grid[None]).to(dev)
    sh = _native.shading_arg(g)
    k, ids = RAW[kind]
    L = _native.lib()
    if name == "rgb":
        rc = L.mi_isp_demosaic_directional_raw_batch(_native.ptr_array(srcs), _native.ptr_array(outs), len(srcs), H, W, k, ids,
                                                     code, pattern, lv, sh, _native.ccm_arg(ccm), _native.stream_ptr(dev))
    else:
        rc = L.mi_isp_raw_cfa_batch(_native.ptr_array(srcs), _native.ptr_array(outs), len(srcs), H, W, k, ids, code, lv, sh,
                                    _native.stream_ptr(dev))
    _native.check(rc)
    torch.cuda.synchronize(dev)


# ---- directional() through mi_isp_demosaic_directional_cfa ----------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("pattern", [0, 1, 2, 3])
def test_directional_cfa(ti, dev, planes, work, pattern):
    """Every output dtype, with and without a matrix, at every shape."""
    for k, shape in enumerate(R.SHAPES):
        cfa = R.stripes_cfa(shape, k % 4, O.NP_DTYPE[work])
        base = planes(cfa, pattern)
        t = torch.from_numpy(cfa).to(dev)
        for out in OUTS:
            for ccm in (None, CCM):
                got = ti.demosaic.directional(t, ti.BayerPattern(pattern), ccm, dtype=out)
                assert got.device == dev and got.shape == shape + (3,)
                assert_exact(got.cpu().numpy(), R.finish(base, ccm, out), f"{work} p{pattern} {shape} -> {out} ccm={ccm is not None}")
        host = ti.demosaic.directional(cfa, ti.BayerPattern(pattern))          # numpy in, numpy out, the CFA's dtype
        assert isinstance(host, np.ndarray)
        assert_exact(host, R.finish(base, None, work), "numpy round trip")


@pytest.mark.parametrize("work", ["f16", "f32"])
def test_directional_cfa_views(ti, dev, planes, work):
    """A non-contiguous CFA (a column window of a wider buffer) and a contiguous one at an odd element offset of its storage."""
    H, W = R.SHAPES[-1]
    cfa = R.stripes_cfa((H, W), 1, O.NP_DTYPE[work])
    want = R.finish(planes(cfa, O.GRBG), CCM, work)
    wide = torch.zeros((H, W + 6), dtype=torch.from_numpy(cfa).dtype, device=dev)
    wide[:, 3:W + 3] = torch.from_numpy(cfa).to(dev)
    view = wide[:, 3:W + 3]
    assert not view.is_contiguous()
    assert_exact(ti.demosaic.directional(view, ti.BayerPattern.GRBG, CCM).cpu().numpy(), want, f"{work} column window")
    flat = torch.zeros(H * W + 5, dtype=wide.dtype, device=dev)
    flat[3:3 + H * W] = torch.from_numpy(cfa).to(dev).reshape(-1)
    odd = flat[3:3 + H * W].view(H, W)
    assert odd.is_contiguous() and odd.storage_offset() == 3
    assert_exact(ti.demosaic.directional(odd, ti.BayerPattern.GRBG, CCM).cpu().numpy(), want, f"{work} odd offset")
    with pytest.raises(ValueError):
        ti.demosaic.directional(torch.zeros((4, 4), dtype=torch.uint8, device=dev))


# ---- the raw entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_raw_batch_and_raw_cfa(ti, rng, dev, planes, work, kind):
    """Every (kind, work dtype): plain, and with per-site blacks and a per-site grid; the image against the restatement
    applied to the loaders' CFA, the decode-only kernel against that CFA."""
    tdt = torch.float16 if work == "f16" else torch.float32
    for k, shape in enumerate([R.SHAPES[-1], R.SHAPES[-2], (2, 6)]):
        for extras in (False, True):
            pattern = (k + 2 * extras) % 4
            src, x, black, white, ccm = source(kind, shape, k, levels=extras)
            grid = make_grid(rng, 5, 7, 4) if extras else None
            cfa = route_cfa(x, grid, work)
            R.assert_covered(cfa if kind != "16f" else (cfa.astype(f32) / f32(4096)).astype(cfa.dtype), pattern, f"{kind} {shape}")
            t = torch.from_numpy(src).to(dev)
            what = f"{kind} {work} {shape} p{pattern} extras={extras}"
            rgb = torch.empty(shape + (3,), dtype=tdt, device=dev)
            raw_call("rgb", [t], [rgb], shape, kind, work, pattern, black, white, grid, ccm, dev)
            assert_exact(rgb.cpu().numpy(), R.finish(planes(cfa, pattern), ccm, work), what + " image")
            out = torch.empty(shape, dtype=tdt, device=dev)
            raw_call("cfa", [t], [out], shape, kind, work, pattern, black, white, grid, None, dev)
            assert_exact(out.cpu().numpy(), cfa, what + " CFA")


@pytest.mark.parametrize("work", ["f16", "f32"])
def test_raw_batch_frames(ti, rng, dev, planes, work):
    """Three frames in one launch, and 34 frames: more than one launch takes (32)."""
    tdt = torch.float16 if work == "f16" else torch.float32
    grid = make_grid(rng, 3, 4, 1)
    for shape, n in ((R.SHAPES[-2], 3), ((6, 4), 34)):
        srcs = [source("p12", shape, seed, levels=True) for seed in range(n)]
        black, white = srcs[0][2:4]
        ts = [torch.from_numpy(s[0]).to(dev) for s in srcs]
        rgbs = [torch.empty(shape + (3,), dtype=tdt, device=dev) for _ in srcs]
        cfas = [torch.empty(shape, dtype=tdt, device=dev) for _ in srcs]
        raw_call("rgb", ts, rgbs, shape, "p12", work, O.BGGR, black, white, grid, CCM, dev)
        raw_call("cfa", ts, cfas, shape, "p12", work, O.BGGR, black, white, grid, None, dev)
        for i, s in enumerate(srcs):
            cfa = route_cfa(s[1], grid, work)
            assert_exact(cfas[i].cpu().numpy(), cfa, f"{work} {shape} frame {i} of {n} CFA")
            assert_exact(rgbs[i].cpu().numpy(), R.finish(planes(cfa, O.BGGR), CCM, work), f"{work} {shape} frame {i} of {n}")


# ---- the ISP ----------------------------------------------------------------------------------------------------------
def expected_image(isp, cfa, pattern, work, planes):
    H, W = cfa.shape
    rgb = R.finish(planes(cfa, pattern), isp.color_correct_matrix, work)
    sz = O.isp_output_size(H, W, isp.resize_width, None)
    return rgb if sz is None else O.resize_bilinear(rgb, sz[0], sz[1])


@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_loader(ti, rng, dev, monkeypatch, planes, cam, work, kind):
    """Every loader with the option on, with and without resize_width, levels and a grid: the CFA at _process_image (the
    routes that have one) is the one the ISP without the option hands over, the image is the restatement of the route's
    CFA, resized."""
    shape = R.SHAPES[-1]
    for k, resize in enumerate((0, 48)):
        pattern = (k + 1) % 4
        src, x, black, white, ccm = source(kind, shape, k, levels=bool(k))
        grid = make_grid(rng, 5, 7, 4) if k else None
        kw = dict(device=dev, correct_colors=True, color_correction=ccm, black_level=black, white_level=white,
                  lens_shading=grid, resize_width=resize)
        isp = getattr(ti, cam)(ti.BayerPattern(pattern), demosaic=ti.Demosaic("directional"), **kw)
        assert isp.demosaic == ti.Demosaic("directional")
        got = capture(monkeypatch, isp)
        t = torch.from_numpy(src).to(dev)
        img = call(isp, kind, t)
        assert getattr(img, "_mi_metering_sub", None) is None, "the images carry no subsample tag"
        cfa = route_cfa(x, grid, work)
        what = f"{cam} {kind} p{pattern} resize={resize}"
        if kind in ("16u", "16f", "32f"):                                      # (the routes with a CFA)
            assert_exact(got[0].cpu().numpy(), cfa, what + " CFA")
        else:
            assert not got, "a packed frame without a map goes straight from the packed bytes"
        assert_exact(img.cpu().numpy(), expected_image(isp, cfa, pattern, work, planes), what + " image")


@pytest.mark.parametrize("cam,work", CAMS)
def test_raw_stage_defect_map_and_lens(ti, rng, dev, monkeypatch, planes, cam, work):
    shape = H, W = R.SHAPES[-1]
    pattern = O.GBRG
    src, x, black, white, ccm = source("p12", shape, 2)
    t = torch.from_numpy(src).to(dev)
    kw = dict(device=dev, correct_colors=True, color_correction=ccm, resize_width=48)
    on = ti.Demosaic("directional")
    # a raw stage on: the chain's CFA as without the option, demosaiced by the directional kernel
    hl = ti.Highlights("rebuild", 0.7)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), demosaic=on, highlights=hl, **kw)
    off = getattr(ti, cam)(ti.BayerPattern(pattern), highlights=hl, **kw)
    got = capture(monkeypatch, isp)
    img = isp.load_packed12(t).cpu().numpy()
    off.load_packed12(t)
    assert len(got) == 2
    assert_exact(got[0].cpu().numpy(), got[1].cpu().numpy(), f"{cam} highlights CFA")
    assert_exact(img, expected_image(isp, got[0].cpu().numpy(), pattern, work, planes), f"{cam} highlights image")
    # a defect map on a packed frame, no raw stage: decode, fix-up, demosaic
    m = ti.DefectMap([(0, 0), (30, 31), (31, 64), (32, 63), (65, 129), (33, 0)], shape)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), demosaic=on, **kw)
    got.clear()
    n_cfa = _count_calls(monkeypatch, "mi_isp_raw_cfa_batch")
    imgs = isp.load_packed12_batch([t, t], defects=[m, None])
    assert len(n_cfa) == 1 and len(got) == 1
    want = correct_cfa(route_cfa(x, None, work), m.mask(), work)
    assert_exact(got[0].cpu().numpy(), want, f"{cam} defect map CFA")
    assert_exact(imgs[0].cpu().numpy(), expected_image(isp, want, pattern, work, planes), f"{cam} defect map image")
    assert_exact(imgs[1].cpu().numpy(), expected_image(isp, route_cfa(x, None, work), pattern, work, planes), f"{cam} frame without a map")
    # a lens: the remap of the full-resolution directional image
    K = np.array([[120.0, 0, W / 2 - 3], [0, 124.0, H / 2 + 2], [0, 0, 1]])
    lens = ti.LensDistortion(K, (-0.2, 0.05, 0.001, -0.002), shape)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), demosaic=on, device=dev, correct_colors=True, color_correction=ccm, scale=0.5)
    img = isp.load_packed12(t, undistort=lens)
    full = torch.from_numpy(R.finish(planes(route_cfa(x, None, work), pattern), isp.color_correct_matrix, work)).to(dev)
    assert_exact(img.cpu().numpy(), isp._undistort([full], [lens], H, W)[0].cpu().numpy(), f"{cam} lens image")


def test_process_packed12_takes_the_two_calls(ti, dev):
    shape = (64, 64)
    frames = [torch.from_numpy(source("p12", shape, s)[0]).to(dev) for s in range(3)]
    kw = dict(device=dev, moving_alpha=0.3, correct_colors=True, demosaic=ti.Demosaic("directional"))
    a, b = ti.Camera16(ti.BayerPattern.RGGB, **kw), ti.Camera16(ti.BayerPattern.RGGB, **kw)
    for _ in range(2):
        outs = a.process_packed12(frames, gamma=0.8)
        want = b.tonemap_reinhard(b.load_packed12_batch(frames), gamma=0.8)
        for o, w in zip(outs, want):
            assert torch.equal(o, w)
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), "metering")
    plain = ti.Camera16(ti.BayerPattern.RGGB, device=dev, moving_alpha=0.3, correct_colors=True)
    assert not torch.equal(plain.process_packed12(frames, gamma=0.8)[0], outs[0]), "the option must change the image"


@pytest.mark.parametrize("batch", [False, True])
def test_route_of_packed_frames(ti, dev, monkeypatch, batch):
    """Packed frames with no raw stage and no map: ONE directional launch for the call, no 13-tap demosaic, no packed load."""
    from taichi_image_amd import _native
    shape = R.SHAPES[-2]
    frames = [torch.from_numpy(source("p12", shape, s)[0]).to(dev) for s in range(3 if batch else 1)]
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, resize_width=32, demosaic=ti.Demosaic("directional"))
    n_dir = _count_calls(monkeypatch, "mi_isp_demosaic_directional_raw_batch")
    others = [_count_calls(monkeypatch, n) for n in _native.SIGNATURES
              if n == "mi_isp_demosaic" or n.startswith("mi_isp_load_packed") and "is_fused" not in n and "supported" not in n]
    assert len(others) >= 10
    if batch:
        isp.load_packed12_batch(frames)
    else:
        isp.load_packed12(frames[0])
    assert len(n_dir) == 1 and not any(others)


@pytest.mark.parametrize("cam,work", CAMS)
def test_option_off_gives_the_bits_of_today(ti, rng, dev, cam, work):
    """demosaic=None, Demosaic("malvar") and set(demosaic=False): the loaders' bits are the oracle's 13-tap ones."""
    shape = R.SHAPES[-1]
    src = source("p12", shape, 3)[0]
    t = torch.from_numpy(src).to(dev)
    want = O.isp_load_packed12(src, work, resize_width=48)
    none = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, resize_width=48)
    malvar = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, resize_width=48, demosaic=ti.Demosaic("malvar"))
    turned = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, resize_width=48, demosaic=ti.Demosaic("directional"))
    assert not np.array_equal(turned.load_packed12(t).cpu().numpy(), want), "the option must change the image"
    turned.set(moving_alpha=0.2)                                              # (None leaves it)
    assert turned.demosaic is not None
    turned.set(demosaic=False)
    assert turned.demosaic is None and none.demosaic is None and malvar.demosaic.method == "malvar"
    for isp in (none, malvar, turned):
        assert_exact(isp.load_packed12(t).cpu().numpy(), want, f"{cam} option off")
        assert_exact(isp.load_packed12_batch([t, t])[1].cpu().numpy(), want, f"{cam} option off, batch")
    with pytest.raises(ValueError):
        turned.set(demosaic="directional")
