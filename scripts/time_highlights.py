"""The cost of highlight reconstruction: load_packed12_batch on six 4096 x 3072 Camera16 frames, highlights off, "rebuild"
and "clip", on frames with about 0 %, 5 % and 100 % clipped pixels (the highlights launch, then the demosaic of the
reconstructed CFAs), then the highlights kernel alone (mi_isp_highlights_raw_batch, one launch for the six frames) against
the raw noise reduction kernel at radius 1 (mi_isp_denoise_raw_batch) on the same frames, and against a one-launch device
copy that moves the same number of bytes (packed 12-bit frame in, f16 CFA out: 3.5 bytes per pixel, copied as 1.75 read and
1.75 written), all in the same run.  HIP-event time per call, best of three rounds, in us per frame."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
H, W = 3072, 4096
CLIP = 0.98


SCENES = [np.minimum(np.rint(synthetic.mosaic_rggb(synthetic.synthetic_scene(i, H, W)).astype(np.float64) * 4095),
                     int(0.9 * 4095)).astype(np.uint16) for i in range(6)]     # (below the clip level)


def frames(fraction):
    """Six packed frames with about `fraction` of their pixels at the white level, in 32 x 32 blobs (1.0: every pixel)."""
    out, share = [], 0.0
    rng = np.random.default_rng(7)
    for v12 in SCENES:
        codes = v12.copy()
        if fraction >= 1.0:
            codes[...] = 4095
        elif fraction > 0:
            n = int(fraction * H * W / 1024)
            for r, c in zip(rng.integers(0, H - 32, n), rng.integers(0, W - 32, n)):
                codes[r:r + 32, c:c + 32] = 4095
        share += float((codes.astype(np.float32) * np.float32(1 / 4095) >= np.float32(CLIP)).mean()) / 6
        out.append(torch.from_numpy(synthetic.pack12(codes)).to(dev))
    return out, share


def timed(fn, n=40, warm=5):
    for _ in range(warm): fn()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / n * 1e3)
    return best


L = _native.lib()
stream = _native.stream_ptr(dev)
SETTINGS = {"off": None, "rebuild": ti.Highlights("rebuild", CLIP), "clip": ti.Highlights("clip", CLIP)}
nbytes = H * W * 3 // 2 + H * W * 2                       # packed frame read once, f16 CFA written once
slower = []
for fraction in (0.0, 0.05, 1.0):
    fr, share = frames(fraction)
    print(f"--- frames with {share * 100:.1f} % clipped pixels")
    base = None
    for name, hl in SETTINGS.items():
        isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, highlights=hl)
        us = timed(lambda: isp.load_packed12_batch(fr)) / 6
        base = us if base is None else base
        print(f"load_packed12_batch, highlights {name:7s}: {us:7.2f} us per frame ({(us / base - 1) * 100:+.1f} % against off)")
    cfas = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in fr]
    srcs, outs = _native.ptr_array(fr), _native.ptr_array(cfas)
    kernel = {}
    for name in ("rebuild", "clip"):
        arg = SETTINGS[name]._arg((1.8, 1.0, 2.1))
        launch = lambda: _native.check(L.mi_isp_highlights_raw_batch(srcs, outs, 6, H, W, _native.MI_RAW_PACKED12, 0,  # noqa
                                                                     _native.MI_F16, 0, None, None, None, arg, 0, stream))
        kernel[name] = timed(launch) / 6
    dn = ti.RawDenoise(0.002, 0.006, radius=1)._arg()
    launch = lambda: _native.check(L.mi_isp_denoise_raw_batch(srcs, outs, 6, H, W, _native.MI_RAW_PACKED12, 0,  # noqa
                                                              _native.MI_F16, None, None, None, dn, stream))
    kernel["denoise R=1"] = timed(launch) / 6
    a = torch.empty(6 * nbytes // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    kernel["device copy"] = timed(lambda: b.copy_(a)) / 6
    for name, us in kernel.items():
        print(f"kernel alone, {name:11s}, six frames in one launch: {us:6.2f} us per frame, "
              f"{nbytes / (us * 1e-6) / 1e9:7.1f} GB/s")
    for name in ("rebuild", "clip"):
        if not kernel[name] < kernel["denoise R=1"]:
            slower.append(f"{name} at {share * 100:.0f} % clipped: {kernel[name]:.2f} us against {kernel['denoise R=1']:.2f} us")
print("the highlights kernel takes less time than the denoise kernel at radius 1 on the same frames: "
      + ("yes, in every case" if not slower else "NO - " + "; ".join(slower)))
sys.exit(1 if slower else 0)
