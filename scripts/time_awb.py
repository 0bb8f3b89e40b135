"""The cost of auto white balance: load_packed12_batch on six 4096 x 3072 Camera16 frames, full size (the stream kernel)
and with resize_width=1920 (config 3: the fused resize kernel), AWB off and on (the load through the effective 2 x 2
grid plus the statistics launch), then the statistics kernel alone (mi_isp_awb_stats_packed, one launch for the six
frames) and the update kernel alone (mi_isp_awb_update).  HIP-event time per call, best of three rounds."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
fr = [torch.from_numpy(synthetic.synthetic_packed12(i)).to(dev) for i in range(6)]


def timed(fn, n=60, warm=8):
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
    for awb in (False, True):
        isp = ti.Camera16(ti.BayerPattern.RGGB, resize_width=rw, device=dev, auto_white_balance=awb)
        us = timed(lambda: isp.load_packed12_batch(fr)) / 6
        base = us if base is None else base
        print(f"resize_width={rw:4d} awb={'on' if awb else 'off':3s}: {us:6.2f} us per frame "
              f"({(us / base - 1) * 100:+.1f} % against AWB off)")
L = _native.lib()
isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, auto_white_balance=True)
ptrs = _native.ptr_array(fr)
stream = _native.stream_ptr(dev)
stats = lambda: _native.check(L.mi_isp_awb_stats_packed(ptrs, 6, 3072, 4096, 12, 0, None, None, 0.95, 0.02, 4,   # noqa
                                                        isp._awb_pending.data_ptr(), stream))
print(f"statistics kernel alone, six frames in one launch: {timed(stats):6.2f} us per call")
print(f"update kernel alone (2 x 2 grid): {timed(isp.update_white_balance):6.2f} us per call")
