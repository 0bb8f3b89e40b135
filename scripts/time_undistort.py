"""The cost of lens distortion correction: load_packed12_batch on six 4096 x 3072 Camera16 frames, full size and with
resize_width=1920, without a lens and with a different analytic lens per camera (the rational model), and the remap
alone (interpolate.undistort of one loaded f16 frame) with its algorithmic rate: one source read plus the output write.
HIP-event time per frame, best of three rounds."""
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


def lens(k):
    K = np.array([[2900.0 + 10 * k, 0, 2048.3 - k], [0, 2895.0 + 7 * k, 1535.6 + k], [0, 0, 1]])
    return ti.LensDistortion(K, (-0.36, 0.19, 0.0035, -0.0021, -0.05, 0.03, 0.012, -0.005), (H, W))


lenses = [lens(k) for k in range(6)]
for rw in (0, 1920):
    isp = ti.Camera16(ti.BayerPattern.RGGB, resize_width=rw, device=dev)
    base = timed(lambda: isp.load_packed12_batch(fr)) / 6
    us = timed(lambda: isp.load_packed12_batch(fr, undistort=lenses)) / 6
    print(f"resize_width={rw:4d}: load_packed12_batch {base:7.2f} us per frame without a lens, {us:7.2f} with one "
          f"({(us / base - 1) * 100:+.1f} %)")
img = ti.Camera16(ti.BayerPattern.RGGB, device=dev).load_packed12(fr[0])
for name, ln in (("analytic, rational", lenses[0]),
                 ("table", ti.LensDistortion.from_map(lenses[0].distortion_map(H, W), (H, W)))):
    us = timed(lambda: ti.interpolate.undistort(img, ln), n=100)
    nbytes = 2 * H * W * 3 * 2
    print(f"remap alone ({name}), 4096 x 3072 f16 -> f16: {us:7.2f} us, {nbytes / us / 1e6:5.2f} TB/s algorithmic "
          f"(2 x {H * W * 6 / 1e6:.1f} MB)")
