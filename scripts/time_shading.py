"""The cost of lens shading in the load kernels: load_packed12_batch on six 4096 x 3072 Camera16 frames, full size
(the stream kernel) and with resize_width=1920 (config 3: the fused resize kernel), each without a grid and with a 17 x 13
per-site grid, without and with per-site levels.  HIP-event time per step, best of three rounds."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import synthetic
dev = torch.device("cuda", 0)
fr = [torch.from_numpy(synthetic.synthetic_packed12(i)).to(dev) for i in range(6)]
y, x = np.linspace(-1, 1, 17)[:, None], np.linspace(-1, 1, 13)[None, :]
grid = np.stack([1.0 + (0.6 + 0.1 * s) * (y * y + x * x) / 2 for s in range(4)]).astype(np.float32)


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
    for levels in (None, [64, 66, 65, 64]):
        for shading in (None, grid):
            isp = ti.Camera16(ti.BayerPattern.RGGB, resize_width=rw, device=dev, black_level=levels, lens_shading=shading)
            us = timed(lambda: isp.load_packed12_batch(fr)) / 6
            base = us if base is None else base
            print(f"resize_width={rw:4d} levels={'per-site' if levels else 'none':8s} "
                  f"grid={'17x13x4' if shading is not None else 'none':7s}: {us:6.2f} us per frame "
                  f"({(us / base - 1) * 100:+.1f} % against no levels, no grid)")
