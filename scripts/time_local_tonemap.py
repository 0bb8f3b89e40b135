"""The cost of local tone mapping: the operator (mi_isp_local_tonemap_batch, three launches for six images, in place) on
f16 and f32 images at 4096 x 3072 and 1920 x 1440, on a natural scene and on a flat image (every lane of a wave in one bin),
against a one-launch device copy of the six images (the operator reads the image twice and writes it once: 1.5 x the copy
is the floor of the two image passes); then load_packed12_batch per frame with the stage off and on.  HIP-event time per
call, best of three rounds of 40 calls after 5 warm-up calls, with the worst round, in us per image.

    python scripts/time_local_tonemap.py            the table
    python scripts/time_local_tonemap.py --trace    ten calls on the 4096 x 3072 scene per dtype and nothing else, for a
                                                    kernel trace (rocprofv3 --kernel-trace --stats -- python ... --trace):
                                                    the three kernels' own times"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
from taichi_image_amd import local_tonemap as ltm
dev = torch.device("cuda", 0)
TRACE = "--trace" in sys.argv


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
s = ti.LocalTonemap()                                  # strength 0.5, cell 32, 16 bins
for H, W in ((3072, 4096),) if TRACE else ((3072, 4096), (1440, 1920)):
    print(f"--- {W} x {H}, {s}")
    fr = [torch.from_numpy(synthetic.synthetic_packed12(i, H, W)).to(dev) for i in range(6)]
    for cam, work in ((ti.Camera16, "f16"), (ti.Camera32, "f32")):
        off = cam(ti.BayerPattern.RGGB, device=dev, correct_colors=True)
        scene = [im.clone() for im in off.load_packed12_batch(fr)]
        flat = [torch.full_like(im, 0.05) for im in scene]
        nbytes = scene[0].numel() * scene[0].element_size()
        # the operator works in place and its gain is >= 1, so repeated calls on one image would walk every pixel up to
        # white: each timed call first restores the six images (views of one buffer) with ONE device copy - the yardstick
        # itself - and the operator's cost is the difference to the copy alone
        buf = torch.empty((6,) + tuple(scene[0].shape), dtype=scene[0].dtype, device=dev)
        ims = [buf[i] for i in range(6)]
        cb = None
        for name, keep in (("scene", torch.stack(scene)), ("flat", torch.stack(flat))):
            if TRACE:
                if name != "scene":
                    continue
                for _ in range(10):
                    buf.copy_(keep)
                    ltm.apply(ims, s)
                torch.cuda.synchronize()
                continue
            if cb is None:
                cb, cw = timed(lambda: buf.copy_(keep))
                print(f"device copy of the six {work} images, one launch:          {cb / 6:6.2f} us per image (worst round "
                      f"{cw / 6:6.2f}), {2 * nbytes / (cb / 6 * 1e-6) / 1e9:7.1f} GB/s")

            def both():
                buf.copy_(keep)
                ltm.apply(ims, s)
            best, worst = timed(both)
            print(f"copy + operator, {work} {name:5s}, six images in one call:   {best / 6:6.2f} us per image (worst round "
                  f"{worst / 6:6.2f}); operator alone {(best - cb) / 6:6.2f} us per image = {(best - cb) / cb:.2f} x the copy "
                  f"(the aim: 1.5), {3 * nbytes / ((best - cb) / 6 * 1e-6) / 1e9:7.1f} GB/s of its 3 x {nbytes // (H * W)} B per pixel")
        if TRACE:
            continue
        del buf, ims
        base = None
        for name, st in (("off", None), ("on", s)):
            isp = cam(ti.BayerPattern.RGGB, device=dev, correct_colors=True, local_tonemap=st)
            best, worst = timed(lambda: isp.load_packed12_batch(fr))
            base = best if base is None else base
            print(f"load_packed12_batch {work}, local tone mapping {name:3s}: {best / 6:7.2f} us per frame (worst round {worst / 6:7.2f}; "
                  f"{(best - base) / 6:+.2f} us against off)")
