"""The cost of the 3D colour LUT, median us per image.
(a) The operator alone (mi_isp_color_lut_rgb_batch_path, six images in one launch, outputs allocated once) on six 3072 x 4096
    and six 1440 x 1920 u8 RGB images at N = 17, 33 and 65, the table in LDS ("lds") and read through L2 ("global") in the
    same run, beside a device-to-device copy_ of the same bytes read and written as one launch (a stacked tensor, "copy_",
    what the ratios refer to) and beside output sharpening at radius 2 on the same images.  The gathers' bank conflicts and
    cache hits depend on the data, so every figure is taken twice: on a natural scene (the ISP's own u8 outputs of the
    synthetic frames: neighbouring pixels hit equal or adjacent entries) and on random bytes (every gather somewhere else:
    the worst case).  "N=33 lds in place" is the call as the ISP makes it (src == dst).
(b) What color_lut= adds per frame to tonemap_reinhard on six full-resolution Camera16 images (write_back=False, so that
    every call sees the same images), to config 3 (load_packed12_batch with resize_width=1920, then tonemap_reinhard) and to
    process_packed12, each against the same call without it.
The variants of one table alternate within every round; a round times each variant over enough calls to fill WINDOW seconds
between two device events, after a warm-up; the figure is the median over the rounds (min .. max beside it).
`python scripts/time_color_lut.py a` runs part (a) alone (the run to put under a kernel trace)."""
import os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
WINDOW, ROUNDS = 0.2, 7
LDS, GLOBAL = 1, 2


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps          # seconds per call


def table(variants, images):
    """{name: (median, min, max) us per image} of the calls `variants` ({name: fn}), alternating."""
    reps = {}
    for name, fn in variants.items():
        for _ in range(5): fn()
        reps[name] = max(3, int(WINDOW / timed(fn, 3)) + 1)
    got = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            got[name].append(timed(fn, reps[name]) * 1e6 / images)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def show(title, res, base):
    print(title)
    for name, (med, lo, hi) in res.items():
        rel = "" if name == base else f"  {med / res[base][0]:5.2f} x {base}  ({med - res[base][0]:+7.2f} us)"
        print(f"  {name:18s} {med:8.2f} us per image  ({lo:.2f} .. {hi:.2f}){rel}")
    sys.stdout.flush()


def look(n):
    """A smooth look: per-channel gammas and less saturation."""
    k = np.arange(n) / (n - 1)
    r, g, b = np.meshgrid(k, k, k, indexing="ij")
    r, g, b = r ** 0.8, g ** 1.1, 0.05 + 0.9 * b ** 1.3
    l = 0.3 * r + 0.6 * g + 0.1 * b
    return ti.ColorLut(np.stack([l + 0.6 * (c - l) for c in (r, g, b)], -1))


LUTS = {n: look(n) for n in (17, 33, 65)}
frames = [torch.from_numpy(synthetic.synthetic_packed12(i)).to(dev) for i in range(6)]

# (a) the operator against a copy and against sharpening
L = _native.lib()
stream = _native.stream_ptr(dev)
g = torch.Generator(device="cpu").manual_seed(1)
for H, W, kw in ((3072, 4096, {}), (1440, 1920, {"resize_width": 1920})):
    isp = ti.Camera16(ti.BayerPattern.RGGB, device=dev, **kw)
    scene = isp.tonemap_reinhard(isp.load_packed12_batch(frames), gamma=0.6)
    assert tuple(scene[0].shape) == (H, W, 3)
    del isp
    for content in ("scene", "random"):
        srcs = scene if content == "scene" else [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
                                                 for _ in range(6)]
        dsts = [torch.empty_like(s) for s in srcs]
        work = [s.clone() for s in srcs]                  # (the in-place variant's images: their content drifts, harmlessly)
        ps, pd, pw = _native.ptr_array(srcs), _native.ptr_array(dsts), _native.ptr_array(work)
        stack_src = torch.stack(srcs)                     # the same bytes as one tensor: the copy as ONE launch, like the operator
        stack_dst = torch.empty_like(stack_src)

        def copy():
            stack_dst.copy_(stack_src)

        def sharpen(arg=ti.Sharpen(1.5, 2)._arg()):
            _native.check(L.mi_isp_sharpen_rgb_batch(ps, pd, 6, H, W, arg, stream))

        def lut(n, path, a=ps, b=pd):
            t, arg = LUTS[n]._device_table(dev).data_ptr(), LUTS[n]._arg()
            return lambda: _native.check(L.mi_isp_color_lut_rgb_batch_path(a, b, 6, H, W, t, arg, path, stream))

        variants = {"copy_": copy, "sharpen R=2": sharpen}
        for n in (17, 33):
            variants[f"N={n} lds"] = lut(n, LDS)
            variants[f"N={n} global"] = lut(n, GLOBAL)
        variants["N=65 global"] = lut(65, GLOBAL)
        variants["N=33 lds in place"] = lut(33, LDS, pw, pw)
        res = table(variants, 6)
        show(f"(a) operator alone, six {H} x {W} u8 RGB images per call ({H * W * 6 / 1e6:.1f} MB read + written per image), "
             f"{content}", res, "copy_")
        for n in (17, 33):
            print(f"  N={n}: lds / global = {res[f'N={n} lds'][0] / res[f'N={n} global'][0]:.2f}")
        del srcs, dsts, work, stack_src, stack_dst
    del scene

if sys.argv[1:] == ["a"]:
    sys.exit(0)

# (b) what color_lut= adds to the ISP's calls
SETTINGS = {"off": None, "N=17": LUTS[17], "N=33": LUTS[33], "N=65": LUTS[65]}


def isps(**kw):
    return {name: ti.Camera16(ti.BayerPattern.RGGB, device=dev, color_lut=s, **kw) for name, s in SETTINGS.items()}


cams = isps()
images = {name: isp.load_packed12_batch(frames) for name, isp in cams.items()}
show("(b) tonemap_reinhard(write_back=False), six 3072 x 4096 Camera16 images",
     table({n: (lambda n=n: cams[n].tonemap_reinhard(images[n], write_back=False)) for n in cams}, 6), "off")
del images
cams3 = isps(resize_width=1920)
show("(b) config 3: load_packed12_batch(resize_width=1920) + tonemap_reinhard, six frames",
     table({n: (lambda n=n: cams3[n].tonemap_reinhard(cams3[n].load_packed12_batch(frames))) for n in cams3}, 6), "off")
show("(b) process_packed12, six 3072 x 4096 frames",
     table({n: (lambda n=n: cams[n].process_packed12(frames)) for n in cams}, 6), "off")
