"""The cost of chromatic aberration correction: the kernel alone (mi_isp_chromatic_raw_batch, one launch for six packed-12
frames, f16 CFA out) against the highlight reconstruction kernel on the same frames with no clipped pixel
(mi_isp_highlights_raw_batch), the raw noise reduction kernel at radius 1 (mi_isp_denoise_raw_batch) and a one-launch
device copy that moves the same number of bytes (packed 12-bit frame in, f16 CFA out: 3.5 bytes per pixel, copied as 1.75
read and 1.75 written), all in the same run; the kernel with one defect map of 0.01 % of the sites, and with settings at
the shift limit (the staged halo follows the largest shift: 6 rows and columns at 3 px, 12 at 7.9 px); then
load_packed12_batch per frame with the stage off and on.  At 4096 x 3072 and at 1440 x 1920.  HIP-event time per call, best
of three rounds of 40 calls after 5 warm-up calls, with the spread of the rounds, in us per frame."""
import math, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)


def timed(fn, n=40, warm=5):
    """(best, worst) of three rounds, us per call."""
    for _ in range(warm): fn()
    rounds = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / n * 1e3)
    return min(rounds), max(rounds)


L = _native.lib()
stream = _native.stream_ptr(dev)
for H, W in ((3072, 4096), (1440, 1920)):
    print(f"--- {W} x {H}")
    fr = [torch.from_numpy(synthetic.pack12(np.minimum(np.rint(
        synthetic.mosaic_rggb(synthetic.synthetic_scene(i, H, W)).astype(np.float64) * 4095), int(0.9 * 4095)).astype(np.uint16))).to(dev)
        for i in range(6)]                                  # (below the clip level: no clipped pixel)
    Rn = math.hypot(H / 2, W / 2)
    ca = ti.ChromaticAberration((1 + 1.5 / Rn, 1.0 / Rn, 0.5 / Rn), (1 - 1.0 / Rn, -1.5 / Rn, -0.5 / Rn))
    print("largest shift (red, blue) in raw pixels: %.2f, %.2f" % ca.max_shift((H, W)))
    nbytes = H * W * 3 // 2 + H * W * 2                     # packed frame read once, f16 CFA written once
    cfas = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in fr]
    srcs, outs = _native.ptr_array(fr), _native.ptr_array(cfas)
    rng = np.random.default_rng(7)
    n_def = int(1e-4 * H * W)
    dmap = ti.DefectMap(sorted({(int(r), int(c)) for r, c in zip(rng.integers(0, H, n_def), rng.integers(0, W, n_def))}), (H, W))
    darg = dmap._arg(dev)
    import ctypes
    with_map = (ctypes.c_void_p * 6)(*[ctypes.addressof(darg)] * 6)
    ca_arg = ca._arg((H, W))
    wide = ti.ChromaticAberration((1 + 4.0 / Rn, 2.5 / Rn, 1.4 / Rn), (1 - 3.0 / Rn, -3.5 / Rn, -1.4 / Rn))
    print("largest shift (red, blue) of the settings at the limit: %.2f, %.2f" % wide.max_shift((H, W)))
    wide_arg = wide._arg((H, W))
    hl_arg = ti.Highlights("rebuild", 0.98)._arg((1.8, 1.0, 2.1))
    dn_arg = ti.RawDenoise(0.002, 0.006, radius=1)._arg()
    P12, F16 = _native.MI_RAW_PACKED12, _native.MI_F16
    kernel = {}
    kernel["chromatic"] = timed(lambda: _native.check(L.mi_isp_chromatic_raw_batch(
        srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, ca_arg, 0, stream)))
    kernel["chromatic, defect maps"] = timed(lambda: _native.check(L.mi_isp_chromatic_raw_batch(
        srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, with_map, ca_arg, 0, stream)))
    kernel["chromatic, 7.9 px"] = timed(lambda: _native.check(L.mi_isp_chromatic_raw_batch(
        srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, wide_arg, 0, stream)))
    kernel["highlights"] = timed(lambda: _native.check(L.mi_isp_highlights_raw_batch(
        srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, hl_arg, 0, stream)))
    kernel["denoise R=1"] = timed(lambda: _native.check(L.mi_isp_denoise_raw_batch(
        srcs, outs, 6, H, W, P12, 0, F16, None, None, None, dn_arg, stream)))
    a = torch.empty(6 * nbytes // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    kernel["device copy"] = timed(lambda: b.copy_(a))
    for name, (best, worst) in kernel.items():
        print(f"kernel alone, {name:22s}, six frames in one launch: {best / 6:6.2f} us per frame (worst round {worst / 6:6.2f}), "
              f"{nbytes / (best / 6 * 1e-6) / 1e9:7.1f} GB/s")
    c = kernel["chromatic"][0]
    print(f"chromatic / highlights {c / kernel['highlights'][0]:.2f}, / denoise R=1 {c / kernel['denoise R=1'][0]:.2f}, "
          f"/ device copy {c / kernel['device copy'][0]:.2f}; with defect maps ({n_def} sites each) "
          f"{kernel['chromatic, defect maps'][0] / c:.2f} x without; at the shift limit {kernel['chromatic, 7.9 px'][0] / c:.2f} x")
    base = None
    for name, s in (("off", None), ("on", ca)):
        isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, chromatic_aberration=s)
        best, worst = timed(lambda: isp.load_packed12_batch(fr))
        base = best if base is None else base
        print(f"load_packed12_batch, chromatic aberration {name:3s}: {best / 6:7.2f} us per frame (worst round {worst / 6:7.2f}; "
              f"{(best / base - 1) * 100:+.1f} % against off)")
