"""The cost of raw noise reduction: load_packed12_batch on six 4096 x 3072 Camera16 frames, full size (the stream kernel)
and with resize_width=1920 (config 3: the fused resize kernel), denoise off, radius 1 and radius 2 (the filter launch, then
the demosaic and resize of the filtered CFAs), then the denoise kernel alone (mi_isp_denoise_raw_batch, one launch for the
six frames) in us per frame and GB/s (packed 12-bit frame in, f16 CFA out).  HIP-event time per call, best of three
rounds."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
H, W = 3072, 4096
fr = [torch.from_numpy(synthetic.synthetic_packed12(i)).to(dev) for i in range(6)]
SETTINGS = {"off": None, "R=1": ti.RawDenoise(0.002, 0.006, radius=1), "R=2": ti.RawDenoise(0.002, 0.006, radius=2)}


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


for rw in (0, 1920):
    base = None
    for name, dn in SETTINGS.items():
        isp = ti.Camera16(ti.BayerPattern.RGGB, resize_width=rw, device=dev, raw_denoise=dn)
        us = timed(lambda: isp.load_packed12_batch(fr)) / 6
        base = us if base is None else base
        print(f"resize_width={rw:4d} denoise {name:3s}: {us:7.2f} us per frame ({(us / base - 1) * 100:+.1f} % against off)")
L = _native.lib()
cfas = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in fr]
srcs, outs = _native.ptr_array(fr), _native.ptr_array(cfas)
stream = _native.stream_ptr(dev)
nbytes = H * W * 3 // 2 + H * W * 2                       # packed frame read once, f16 CFA written once
for name in ("R=1", "R=2"):
    arg = SETTINGS[name]._arg()
    launch = lambda: _native.check(L.mi_isp_denoise_raw_batch(srcs, outs, 6, H, W, _native.MI_RAW_PACKED12, 0,  # noqa
                                                              _native.MI_F16, None, None, None, arg, stream))
    us = timed(launch) / 6
    print(f"denoise kernel alone, {name}, six frames in one launch: {us:6.2f} us per frame, "
          f"{nbytes / (us * 1e-6) / 1e9:7.1f} GB/s")
