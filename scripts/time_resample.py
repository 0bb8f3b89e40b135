"""The cost of the antialiased resize: six images per call, both work dtypes, 4096 x 3072 -> 1920 x 1440 and
1920 x 1440 -> 960 x 720, in one run:
  (a) mi_isp_resample_batch with the area, the triangle and the lanczos3 tables (one launch each)
  (b) mi_isp_resize_bilinear on the same images (six launches)
  (c) a one-launch device copy of the bytes (a) moves (source in, output out)
then load_packed12_batch of the ISP at the output width with the option on (area) and off.  HIP-event time per call; the
variants alternate within a round and the best of three rounds counts; in us per image, with the ratios to (b) and (c)."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, resample as rs, synthetic
dev = torch.device("cuda", 0)
N = 6
L = _native.lib()
stream = _native.stream_ptr(dev)
FILTERS = ("area", "triangle", "lanczos3")


def timed(fns, n=30, warm=4, rounds=3):
    """{name: best us per call} of the callables fns, alternated within each round."""
    for fn in fns.values():
        for _ in range(warm): fn()
    best = {k: float("inf") for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(n): fn()
            e1.record(); torch.cuda.synchronize()
            best[k] = min(best[k], e0.elapsed_time(e1) / n * 1e3)
    return best


for (H, W), (Hd, Wd) in (((3072, 4096), (1440, 1920)), ((1440, 1920), (720, 960))):
    scale = Wd / W
    for work, tdt, code in (("f16", torch.float16, _native.MI_F16), ("f32", torch.float32, _native.MI_F32)):
        es = 2 if work == "f16" else 4
        gen = torch.Generator(device=dev).manual_seed(1)
        srcs = [torch.rand((H, W, 3), generator=gen, device=dev, dtype=torch.float32).to(tdt) for _ in range(N)]
        dsts = [torch.empty((Hd, Wd, 3), dtype=tdt, device=dev) for _ in range(N)]
        nbytes = (H * W + Hd * Wd) * 3 * es
        ca = torch.empty(N * nbytes // 2, dtype=torch.uint8, device=dev)
        ca2 = torch.empty_like(ca)

        def resample(f):
            return lambda: rs.apply(srcs, dsts, f, H, W, Hd, Wd, scale, scale, code, code, dev)

        def bilinear():
            for s, d in zip(srcs, dsts):
                _native.check(L.mi_isp_resize_bilinear(s.data_ptr(), d.data_ptr(), H, W, Hd, Wd, scale, scale, code, code, stream))

        fns = {f: resample(f) for f in FILTERS}
        fns.update({"bilinear": bilinear, "copy": lambda: ca2.copy_(ca)})
        taps = {f: rs.taps(f, W, Wd, scale) for f in FILTERS}
        if (H, W) == (3072, 4096):                               # the loaders of config 3's frames
            packed = [torch.from_numpy(synthetic.synthetic_packed12(i, H, W)).to(dev) for i in range(N)]
            Cam = getattr(ti, "Camera16" if work == "f16" else "Camera32")
            on = Cam(ti.BayerPattern.RGGB, device=dev, correct_colors=True, resize_width=Wd, resample=ti.Resample("area"))
            off = Cam(ti.BayerPattern.RGGB, device=dev, correct_colors=True, resize_width=Wd)
            fns.update({"isp_on": lambda: on.load_packed12_batch(packed), "isp_off": lambda: off.load_packed12_batch(packed)})
        us = {k: v / N for k, v in timed(fns).items()}
        print(f"--- {W} x {H} -> {Wd} x {Hd}, work dtype {work}: us per image (six images a call)")
        for f in FILTERS:
            print(f"(a) resample {f:9s} T = {taps[f]:2d}, one launch   {us[f]:8.2f}   {nbytes / us[f] / 1e3:7.1f} GB/s   "
                  f"x{us[f] / us['bilinear']:.2f} of (b)   x{us[f] / us['copy']:.2f} of (c)")
        print(f"(b) resize_bilinear, six launches          {us['bilinear']:8.2f}   {nbytes / us['bilinear'] / 1e3:7.1f} GB/s   "
              f"x{us['bilinear'] / us['copy']:.2f} of (c)")
        print(f"(c) device copy of (a)'s bytes             {us['copy']:8.2f}   {nbytes / us['copy'] / 1e3:7.1f} GB/s")
        if "isp_on" in us:
            print(f"load_packed12_batch, option off            {us['isp_off']:8.2f}")
            print(f"load_packed12_batch, resample area         {us['isp_on']:8.2f}   x{us['isp_on'] / us['isp_off']:.2f} of off")
            del packed, on, off
        del srcs, dsts, ca, ca2
        torch.cuda.empty_cache()
