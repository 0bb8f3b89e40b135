"""The cost of the directional demosaic: six 4096 x 3072 and six 1920 x 1440 frames, both work dtypes, in one run:
  (a) mi_isp_demosaic_directional_cfa on six CFAs (six launches)
  (b) mi_isp_demosaic_directional_raw_batch from packed-12 frames (one launch)
  (c) mi_isp_demosaic, the 13-tap filter, on the same CFAs (six launches)
  (d) mi_isp_load_packed_batch, the fused 13-tap load, on the same packed frames (one launch)
  (e) a one-launch device copy of the bytes (a) and (b) move (CFA or packed frame in, work-dtype image out)
then load_packed12_batch of the ISP with and without the option.  HIP-event time per call; the variants alternate within a
round and the best of three rounds counts; in us per frame, with the ratios to (c), (d) and (e)."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
N = 6
L = _native.lib()
stream = _native.stream_ptr(dev)
CCM = _native.ccm_arg(np.array([[1.75, -0.25, -0.30], [-0.10, 1.40, -0.30], [-0.05, -0.55, 2.10]]))


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


for H, W in ((3072, 4096), (1440, 1920)):
    codes = [np.rint(synthetic.mosaic_rggb(synthetic.synthetic_scene(i, H, W)).astype(np.float64) * 4095).astype(np.uint16)
             for i in range(N)]
    packed = [torch.from_numpy(synthetic.pack12(c)).to(dev) for c in codes]
    for work, tdt, code in (("f16", torch.float16, _native.MI_F16), ("f32", torch.float32, _native.MI_F32)):
        es = 2 if work == "f16" else 4
        cfas = [torch.from_numpy(c.astype(np.float32) * np.float32(1 / 4095)).to(dev).to(tdt) for c in codes]
        rgbs = [torch.empty((H, W, 3), dtype=tdt, device=dev) for _ in range(N)]
        p_packed, p_rgbs = _native.ptr_array(packed), _native.ptr_array(rgbs)
        bytes_a = H * W * es + H * W * 3 * es                   # CFA in, image out
        bytes_b = H * W * 3 // 2 + H * W * 3 * es               # packed frame in, image out
        ca, cb = (torch.empty(N * b // 2, dtype=torch.uint8, device=dev) for b in (bytes_a, bytes_b))
        ca2, cb2 = torch.empty_like(ca), torch.empty_like(cb)

        def a():
            for c, o in zip(cfas, rgbs):
                _native.check(L.mi_isp_demosaic_directional_cfa(c.data_ptr(), o.data_ptr(), H, W, code, code, 0, CCM, stream))

        def b():
            _native.check(L.mi_isp_demosaic_directional_raw_batch(p_packed, p_rgbs, N, H, W, _native.MI_RAW_PACKED12, 0, code, 0,
                                                                  None, None, CCM, stream))

        def c():
            for x, o in zip(cfas, rgbs):
                _native.check(L.mi_isp_demosaic(x.data_ptr(), o.data_ptr(), H, W, code, code, 0, CCM, stream))

        def d():
            _native.check(L.mi_isp_load_packed_batch(p_packed, p_rgbs, None, N, H, W, 12, 0, 0, CCM, code, H, W, 0.0, 8, stream))

        on = getattr(ti, "Camera16" if work == "f16" else "Camera32")(ti.BayerPattern.RGGB, device=dev, correct_colors=True,
                                                                      demosaic=ti.Demosaic("directional"))
        off = getattr(ti, "Camera16" if work == "f16" else "Camera32")(ti.BayerPattern.RGGB, device=dev, correct_colors=True)
        t = timed({"a": a, "b": b, "c": c, "d": d, "e_a": lambda: ca2.copy_(ca), "e_b": lambda: cb2.copy_(cb),
                   "isp_on": lambda: on.load_packed12_batch(packed), "isp_off": lambda: off.load_packed12_batch(packed)})
        us = {k: v / N for k, v in t.items()}
        print(f"--- {W} x {H}, work dtype {work}: us per frame (six frames a call)")
        print(f"(a) directional_cfa, six launches      {us['a']:8.2f}   {bytes_a / us['a'] / 1e3:7.1f} GB/s   "
              f"x{us['a'] / us['c']:.2f} of (c)   x{us['a'] / us['e_a']:.2f} of its copy")
        print(f"(b) directional_raw_batch, one launch  {us['b']:8.2f}   {bytes_b / us['b'] / 1e3:7.1f} GB/s   "
              f"x{us['b'] / us['d']:.2f} of (d)   x{us['b'] / us['e_b']:.2f} of its copy")
        print(f"(c) 13-tap demosaic, six launches      {us['c']:8.2f}   {bytes_a / us['c'] / 1e3:7.1f} GB/s   "
              f"x{us['c'] / us['e_a']:.2f} of its copy")
        print(f"(d) 13-tap load_packed_batch           {us['d']:8.2f}   {bytes_b / us['d'] / 1e3:7.1f} GB/s   "
              f"x{us['d'] / us['e_b']:.2f} of its copy")
        print(f"(e) device copy of (a)'s bytes         {us['e_a']:8.2f}   {bytes_a / us['e_a'] / 1e3:7.1f} GB/s")
        print(f"(e) device copy of (b)'s bytes         {us['e_b']:8.2f}   {bytes_b / us['e_b'] / 1e3:7.1f} GB/s")
        print(f"load_packed12_batch, option off        {us['isp_off']:8.2f}")
        print(f"load_packed12_batch, directional       {us['isp_on']:8.2f}   x{us['isp_on'] / us['isp_off']:.2f} of off")
        del cfas, rgbs, ca, cb, ca2, cb2
        torch.cuda.empty_cache()
