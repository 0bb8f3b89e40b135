"""The cost of defective pixel correction: load_packed12_batch on six 4096 x 3072 Camera16 frames, full size (the stream
kernel) and with resize_width=1920 (the fused resize kernel), with no map and with 0.01 % and 0.1 % of the sites of every
camera defective (a different random map per camera).  The maps are cached on the device by a first call, as in
steady-state use.  HIP-event time per step, best of three rounds."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import synthetic
dev = torch.device("cuda", 0)
H, W = 3072, 4096
fr = [torch.from_numpy(synthetic.synthetic_packed12(i)).to(dev) for i in range(6)]
rng = np.random.default_rng(0)


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
    isp = ti.Camera16(ti.BayerPattern.RGGB, resize_width=rw, device=dev)
    base = None
    for frac in (0.0, 1e-4, 1e-3):
        n = int(round(frac * H * W))
        maps = None if n == 0 else [ti.DefectMap(np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1), (H, W))
                                    for _ in fr]
        us = timed(lambda: isp.load_packed12_batch(fr, defects=maps)) / 6
        base = us if base is None else base
        hd, wd = (1440, 1920) if rw else (H, W)
        listed = 0 if maps is None else sum(m._outputs(dev, hd, wd, rw / W if rw else 0.0)[1] for m in maps) // 6
        print(f"resize_width={rw:4d} defects={frac * 100:5.2f} % ({n:5d} sites, {listed:7d} outputs per camera): "
              f"{us:6.2f} us per frame ({(us / base - 1) * 100:+.1f} % against no map)")
