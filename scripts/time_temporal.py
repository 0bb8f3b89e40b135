"""The cost of temporal noise reduction: the kernel alone (mi_isp_temporal_raw_batch, one launch for six packed-12 frames
with a history each) in three forms - f16 CFA out, the plain-f32 single-write form, and an empty history - against a
one-launch device copy that moves the bytes the first form moves (packed 12-bit frame in, f32 history in, f32 history out,
f16 CFA out: 11.5 bytes per pixel, copied as 5.75 read and 5.75 written), the highlight reconstruction kernel on the same
frames (mi_isp_highlights_raw_batch, no clipped pixel) and the raw noise reduction kernel at radius 1
(mi_isp_denoise_raw_batch), all in the same run; then load_packed12_batch per frame with the stage off and on.  At
4096 x 3072 and at 1920 x 1440.  HIP-event time per call, best of three rounds of 40 calls after 5 warm-up calls, with the
worst round, in us per frame."""
import ctypes, os, sys
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
GAIN, READ_NOISE = 2.4e-4, 1.5e-3
for H, W in ((3072, 4096), (1440, 1920)):
    print(f"--- {W} x {H}")
    rng = np.random.default_rng(7)
    codes = [np.minimum(np.rint(synthetic.mosaic_rggb(synthetic.synthetic_scene(i, H, W)).astype(np.float64) * 4095),
                        int(0.9 * 4095)) for i in range(6)]     # (below the clip level: no clipped pixel)
    fr = [torch.from_numpy(synthetic.pack12(c.astype(np.uint16))).to(dev) for c in codes]
    # the history of each frame: the frame itself plus model noise, a static scene (every weight is in use)
    hin = [torch.from_numpy((c / 4095 + rng.normal(0, 1, c.shape) * np.sqrt(GAIN * c / 4095 + READ_NOISE ** 2)).astype(np.float32)).to(dev)
           for c in codes]
    hout = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in fr]
    cfas = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in fr]
    nbytes = H * W * 3 // 2 + H * W * 4 + H * W * 4 + H * W * 2     # packed in, history in, history out, f16 CFA out
    srcs, p_hin, p_hout, outs = _native.ptr_array(fr), _native.ptr_array(hin), _native.ptr_array(hout), _native.ptr_array(cfas)
    tn = ti.TemporalDenoise(GAIN, READ_NOISE)
    tn_arg = tn._arg()
    hl_arg = ti.Highlights("rebuild", 0.98)._arg((1.8, 1.0, 2.1))
    dn_arg = ti.RawDenoise(0.002, 0.006, radius=1)._arg()
    P12, F16 = _native.MI_RAW_PACKED12, _native.MI_F16
    kernel = {}
    kernel["temporal, f16 CFA out"] = timed(lambda: _native.check(L.mi_isp_temporal_raw_batch(
        srcs, p_hin, p_hout, outs, 6, H, W, P12, 0, F16, None, None, None, tn_arg, 0, stream)))
    kernel["temporal, plain f32"] = timed(lambda: _native.check(L.mi_isp_temporal_raw_batch(
        srcs, p_hin, p_hout, None, 6, H, W, P12, 0, F16, None, None, None, tn_arg, 1, stream)))
    kernel["temporal, empty history"] = timed(lambda: _native.check(L.mi_isp_temporal_raw_batch(
        srcs, None, p_hout, outs, 6, H, W, P12, 0, F16, None, None, None, tn_arg, 0, stream)))
    kernel["highlights"] = timed(lambda: _native.check(L.mi_isp_highlights_raw_batch(
        srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, hl_arg, 0, stream)))
    kernel["denoise R=1"] = timed(lambda: _native.check(L.mi_isp_denoise_raw_batch(
        srcs, outs, 6, H, W, P12, 0, F16, None, None, None, dn_arg, stream)))
    a = torch.empty(6 * nbytes // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    kernel["device copy"] = timed(lambda: b.copy_(a))
    moved = {"temporal, plain f32": nbytes - H * W * 2, "temporal, empty history": nbytes - H * W * 4,
             "highlights": H * W * 7 // 2, "denoise R=1": H * W * 7 // 2}
    for name, (best, worst) in kernel.items():
        nb = moved.get(name, nbytes)
        print(f"kernel alone, {name:24s}, six frames in one launch: {best / 6:6.2f} us per frame (worst round {worst / 6:6.2f}), "
              f"{nb / (H * W):5.2f} B per pixel, {nb / (best / 6 * 1e-6) / 1e9:7.1f} GB/s")
    t = kernel["temporal, f16 CFA out"][0]
    print(f"temporal / device copy {t / kernel['device copy'][0]:.2f} (the aim: 1.5), / highlights "
          f"{t / kernel['highlights'][0]:.2f}, / denoise R=1 {t / kernel['denoise R=1'][0]:.2f}")
    del a, b
    base = None
    for name, s in (("off", None), ("on", tn)):
        isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, temporal_denoise=s)
        hists = None if s is None else [ti.TemporalHistory() for _ in fr]
        best, worst = timed(lambda: isp.load_packed12_batch(fr, history=hists))
        base = best if base is None else base
        print(f"load_packed12_batch, temporal noise reduction {name:3s}: {best / 6:7.2f} us per frame (worst round {worst / 6:7.2f}; "
              f"{(best / base - 1) * 100:+.1f} % against off)")
