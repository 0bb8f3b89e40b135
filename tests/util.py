"""Shared helpers for the parity tests."""
import numpy as np

from oracle import isp_oracle as O

NP = O.NP_DTYPE


def bits(a: np.ndarray) -> np.ndarray:
    """Bit view for exact comparison of float arrays (NaN-safe, -0 != +0)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float16:
        return a.view(np.uint16)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a


def assert_exact(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert got.dtype == ref.dtype, f"{what}: dtype {got.dtype} != {ref.dtype}"
    bad = bits(got) != bits(ref)
    if bad.any():
        idx = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError(f"{what}: {bad.sum()} / {bad.size} elements differ, first at {idx}: "
                             f"got {got[idx]!r} want {ref[idx]!r}")


def assert_close(got, ref, what="", rel=1e-4, max_bad_frac=0.0):
    """The parity contract for floating-point stages: |got - ref| <= rel*|ref| + one unit of the
    output type (1 LSB for integer outputs, 1 ulp for f16/f32 outputs).  NaNs must coincide."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert got.dtype == ref.dtype, f"{what}: dtype {got.dtype} != {ref.dtype}"
    g, r = got.astype(np.float64), ref.astype(np.float64)
    nan_g, nan_r = np.isnan(g), np.isnan(r)
    assert np.array_equal(nan_g, nan_r), f"{what}: NaN pattern differs ({nan_g.sum()} vs {nan_r.sum()})"
    if ref.dtype == np.float16:
        unit = np.maximum(np.abs(r), 2.0 ** -14) * 2.0 ** -10   # one f16 ulp (>= spacing at |r|)
    elif ref.dtype == np.float32:
        unit = np.maximum(np.abs(r), 1e-30) * 2.0 ** -22 + 1e-7
    else:
        unit = 1.0
    err = np.abs(g - r)
    tol = rel * np.abs(r) + unit
    bad = (err > tol) & ~nan_r
    frac = bad.mean() if bad.size else 0.0
    if frac > max_bad_frac:
        idx = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError(f"{what}: {bad.sum()} / {bad.size} outside tolerance (max err {err[~nan_r].max():.4g}), "
                             f"first at {idx}: got {got[idx]!r} want {ref[idx]!r}")
    return float(err[~nan_r].max()) if (~nan_r).any() else 0.0


def _count_calls(monkeypatch, name):
    """Count the calls of one library entry point (the probe that a path was taken)."""
    from taichi_image_amd import _native
    L = _native.lib()
    fn, calls = getattr(L, name), []

    def counted(*args):
        calls.append(name)
        return fn(*args)
    monkeypatch.setattr(L, name, counted)
    return calls


def random_cfa(rng, H, W, dtype):
    if dtype == "u8":
        return rng.integers(0, 256, (H, W)).astype(np.uint8)
    if dtype == "u16":
        return rng.integers(0, 65536, (H, W)).astype(np.uint16)
    x = rng.random((H, W), dtype=np.float32)
    return x.astype(NP[dtype])


def natural_packed12(rng, H, W, pattern=O.RGGB, ids_format=False, dark=0.0):
    """A smooth-plus-noise scene, mosaiced and packed (12 bit)."""
    r = np.arange(H)[:, None] / max(H, 1)
    c = np.arange(W)[None, :] / max(W, 1)
    base = 0.1 + 0.8 * (0.5 + 0.5 * np.sin(6.0 * r + 1.0)) * (0.5 + 0.5 * np.cos(9.0 * c))
    img = np.stack([np.clip(base * g + rng.normal(0, 0.03, (H, W)) - dark, 0, 1) for g in (1.0, 0.8, 0.6)], -1)
    cfa = O.rgb_to_bayer(img.astype(np.float32), pattern)
    v12 = np.rint(cfa.astype(np.float64) * 4095).astype(np.uint16)
    return O.encode12(v12, ids_format=ids_format)


def reuse_case(ti, dev, cam, frames, sequence, alpha=0.3):
    """One list of images through two calls.  The first Reinhard call overwrites every image with its mapped values p
    (camera_isp.py:211); the second call must meter the MUTATED images (camera_isp.py:168-175 reads the tensors it is
    given), not the subsample the load kernel left behind.  The oracle of the second call consumes the device's images
    as they stand after the first (their own parity is asserted first)."""
    import torch
    from oracle import c_oracle
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, moving_alpha=alpha, device=dev)
    st = c_oracle.IspState(alpha)
    imgs = [isp.load_packed12(f) for f in frames]
    refs = [im.cpu().numpy() for im in imgs]
    if sequence == "kernel_then_metering":
        # the static kernel with metrics of the caller's own, as ISP.tonemap_only does (camera_isp.py:387-390)
        isp.update_metering(imgs)
        m1 = st.update_metering(refs)
        assert_close(isp.metrics.cpu().numpy(), m1, "metrics 1", rel=2e-5)
        for k, im in enumerate(imgs):
            out = torch.empty(im.shape, dtype=torch.uint8, device=dev)
            type(isp).reinhard_kernel(im, out, isp.metrics, 0.6, 1.0, 1.0, 0.0)
            ref_u8, ref_after = c_oracle.reinhard_isp(refs[k], m1, gamma=0.6)
            assert_close(out.cpu().numpy(), ref_u8, f"u8 img {k}")
            assert_close(im.cpu().numpy(), ref_after, f"in-place p img {k}")
            assert not hasattr(im, "_mi_metering_sub"), "a subsample taken before the write survived it"
        mut = [im.cpu().numpy() for im in imgs]
        isp.update_metering(imgs)
        assert_close(isp.metrics.cpu().numpy(), st.update_metering(mut), "metrics after ISP.reinhard_kernel", rel=2e-5)
        return
    outs = isp.tonemap_reinhard(imgs, gamma=0.6)
    m1 = st.update_metering(refs)
    assert_close(isp.metrics.cpu().numpy(), m1, "metrics 1", rel=2e-5)
    for k in range(len(imgs)):
        ref_u8, ref_after = c_oracle.reinhard_isp(refs[k], m1, gamma=0.6)
        assert_close(outs[k].cpu().numpy(), ref_u8, f"u8 1 img {k}")
        assert_close(imgs[k].cpu().numpy(), ref_after, f"in-place p 1 img {k}")
    mut = [im.cpu().numpy() for im in imgs]
    assert any(not np.array_equal(a, b) for a, b in zip(mut, refs)), "the first call did not write p back"
    if sequence == "reinhard_twice":
        outs2 = isp.tonemap_reinhard(imgs, gamma=0.8)
        m2 = st.update_metering(mut)
        assert_close(isp.metrics.cpu().numpy(), m2, "metrics 2", rel=2e-5)
        for k in range(len(imgs)):
            ref_u8, ref_after = c_oracle.reinhard_isp(mut[k], m2, gamma=0.8)
            assert_close(outs2[k].cpu().numpy(), ref_u8, f"u8 2 img {k}")
            assert_close(imgs[k].cpu().numpy(), ref_after, f"in-place p 2 img {k}")
    else:
        assert sequence == "reinhard_then_linear"
        outs2 = isp.tonemap_linear(imgs, gamma=0.8)
        m2 = st.update_metering(mut)
        assert_close(isp.metrics.cpu().numpy(), m2, "metrics 2", rel=2e-5)
        for k in range(len(imgs)):
            assert_close(outs2[k].cpu().numpy(), c_oracle.linear_isp(mut[k], m2, 0.8), f"linear 2 img {k}")
    # the stale subsample would have given the metrics of the un-mutated images: make sure the two differ at all
    stale = c_oracle.IspState(alpha)
    stale.update_metering(refs)
    assert not np.allclose(stale.update_metering(refs), m2, rtol=1e-3), "the sequence does not tell stale from fresh"


def scene_cut_state(rng, H, W, bright, work="f16", alpha=0.3):
    """A scene cut: the metering state of a group of the other brightness (`bright=True`: the state of a bright group,
    for a dark group to follow; False: a dark state before a bright group).  Seeded as the previous state, it puts
    pixels of the next group below bmin (scaled < 0) and above bmax (scaled > 1)."""
    frames = [natural_packed12(rng, H, W, dark=(-0.35 if bright else 0.6) + 0.02 * k) for k in range(2)]
    return O.IspState(alpha).update_metering([O.isp_load_packed12(f, work) for f in frames])


def scene_cut_frames(rng, H, W, bright, n=2):
    """The group that follows `scene_cut_state(bright)`: the opposite brightness.  The dark group carries colour patches
    (red and green sites at a ramp of levels, blue sites black): pixels with a channel below bmin and a positive gray,
    whose p < 0 the Reinhard output maps through the gamma curve - visibly for an even 1/gamma."""
    if not bright:
        return [natural_packed12(rng, H, W, dark=-0.4 + 0.03 * k) for k in range(n)]
    frames = []
    for k in range(n):
        v12 = O.decode12(natural_packed12(rng, H, W, dark=0.55 + 0.03 * k), "u16")
        i = 0
        for r0 in range(4, H - 12, 24):
            for c0 in range(4, W - 12, 24):
                patch = v12[r0:r0 + 12, c0:c0 + 12]
                patch[...] = 1500 + (i * 97) % 1500
                patch[1::2, 1::2] = 0
                i += 1
        frames.append(O.encode12(v12))
    return frames


def degenerate_cfa(kind, H, W, rng=None):
    """12-bit CFA frames where the bounds collapse or sit exactly at (0, 1): lens cap, blown out, flat grey card,
    binary 0/4095, one non-black pixel."""
    if kind == "zero":
        return np.zeros((H, W), np.uint16)
    if kind == "full":
        return np.full((H, W), 4095, np.uint16)
    if kind == "flat":
        return np.full((H, W), 1800, np.uint16)
    if kind == "binary":
        rng = rng or np.random.default_rng(5)
        return (rng.random((H, W)) < 0.5).astype(np.uint16) * 4095
    if kind == "one":
        v = np.zeros((H, W), np.uint16)
        v[H // 2, W // 3] = 3000
        return v
    raise ValueError(kind)


DEGENERATE = ["zero", "full", "flat", "binary", "one"]
# 1/gamma in f32 is exactly 2, 4, 3, 1.667, 1 and 0.4545: even and odd integral exponents and non-integral ones
GAMMAS = [0.5, 0.25, 1.0 / 3.0, 0.6, 1.0, 2.2]


def nan_on_grid(img, stride=8, where=((0, 0), (-1, -1)), ch=1):
    """A copy of an (H, W, 3) float image with NaN at sample points of the stride grid (last grid row / column for -1)."""
    out = np.array(img, copy=True)
    H, W = out.shape[:2]
    last_r, last_c = (H - 1) // stride * stride, (W - 1) // stride * stride
    for r, c in where:
        out[last_r if r == -1 else r, last_c if c == -1 else c, ch] = np.nan
    return out


SENTINEL = 0xA5


def u8_batch_with_sentinels(entry, images, H, W, args, dev, in_place=()):
    """One call of the library's u8 batch entry point `entry` (src, dst, n, H, W, *args, stream) on the numpy u8 images (one
    shape), every source and every destination a slot of one device buffer with a run of SENTINEL bytes behind it (slots 16
    bytes aligned, so a W % 4 == 0 image keeps the dword path); the images whose index is in `in_place` are their own
    destination.  Returns the outputs as numpy arrays after asserting that every sentinel run, every source filtered into
    another image and every destination slot of an image filtered in place came back as it went in."""
    import ctypes
    import torch
    from taichi_image_amd import _native
    n, size = len(images), images[0].size
    stride = (size + 64 + 15) // 16 * 16
    host = np.full((n, stride), SENTINEL, np.uint8)
    for k, im in enumerate(images):
        host[k, :size] = im.ravel()
    src = torch.from_numpy(host).to(dev)
    dst = torch.full((n, stride), SENTINEL, dtype=torch.uint8, device=dev)
    sp = [src[k].data_ptr() for k in range(n)]
    dp = [sp[k] if k in in_place else dst[k].data_ptr() for k in range(n)]
    rc = getattr(_native.lib(), entry)((ctypes.c_void_p * n)(*sp), (ctypes.c_void_p * n)(*dp), n, H, W, *args,
                                       _native.stream_ptr(dev))
    _native.check(rc)
    s, d = src.cpu().numpy(), dst.cpu().numpy()
    outs = []
    for k in range(n):
        moved = k not in in_place
        assert (s[k, size:] == SENTINEL).all() and (d[k, size:] == SENTINEL).all(), f"image {k}: bytes behind it were written"
        if moved:
            assert np.array_equal(s[k], host[k]), f"image {k}: its source was written"
        else:
            assert (d[k] == SENTINEL).all(), f"image {k}, filtered in place: its unused slot was written"
        outs.append((d if moved else s)[k, :size].reshape(images[k].shape).copy())
    return outs
