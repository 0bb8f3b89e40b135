"""The cost of luma noise reduction, median us per image.
(a) The operator alone (mi_isp_luma_denoise_rgb_batch, six images in one launch, outputs allocated once) on six 3072 x 4096
    and six 1440 x 1920 u8 RGB images at radius 1, 2 and 3 (the kernel's work does not depend on the data or the thresholds:
    no branch looks at a tap), beside a device-to-device copy_ of the same bytes read and written as one launch (a stacked
    tensor, "copy_", what the ratios refer to), beside output sharpening at radius 2 ("sharpen R=2") and beside chroma noise
    reduction at radius 1 and 2 ("chroma R=1", "chroma R=2") on the same images: the same traffic, one read with a halo and
    one write.  The aims: radius 1 within 1.5 x sharpen R=2, radius 2 within chroma R=2.
(b) What luma_denoise= adds per frame to tonemap_reinhard on six full-resolution Camera16 images (write_back=False, so that
    every call sees the same images) and to config 3 (load_packed12_batch with resize_width=1920, then tonemap_reinhard),
    each against the same call without it.
The variants of one table alternate within every round; a round times each variant over enough calls to fill WINDOW seconds
between two device events, after a warm-up; the figure is the median over the rounds (min .. max beside it).
`python scripts/time_luma_denoise.py a` runs part (a) alone (the run to put under a kernel trace)."""
import os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
WINDOW, ROUNDS = 0.2, 7


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
        print(f"  {name:12s} {med:8.2f} us per image  ({lo:.2f} .. {hi:.2f}){rel}")


# (a) the operator against a copy, sharpening and the chroma filter
L = _native.lib()
stream = _native.stream_ptr(dev)
g = torch.Generator(device="cpu").manual_seed(1)
for H, W in ((3072, 4096), (1440, 1920)):
    srcs = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(6)]
    dsts = [torch.empty_like(s) for s in srcs]
    ps, pd = _native.ptr_array(srcs), _native.ptr_array(dsts)

    stack_src = torch.stack(srcs)                     # the same bytes as one tensor: the copy as ONE launch, like the filter
    stack_dst = torch.empty_like(stack_src)

    def copy():
        stack_dst.copy_(stack_src)

    def sharpen(arg=ti.Sharpen(1.5, 2)._arg()):
        _native.check(L.mi_isp_sharpen_rgb_batch(ps, pd, 6, H, W, arg, stream))

    def chroma(arg):
        return lambda: _native.check(L.mi_isp_chroma_denoise_rgb_batch(ps, pd, 6, H, W, arg, stream))

    def filt(arg):
        return lambda: _native.check(L.mi_isp_luma_denoise_rgb_batch(ps, pd, 6, H, W, arg, stream))

    variants = {"copy_": copy, "sharpen R=2": sharpen, "chroma R=1": chroma(ti.ChromaDenoise(1)._arg()),
                "chroma R=2": chroma(ti.ChromaDenoise(2)._arg())}
    for r in (1, 2, 3):
        variants[f"R={r}"] = filt(ti.LumaDenoise(r, 6, 14)._arg())
    res = table(variants, 6)
    show(f"(a) operator alone, six {H} x {W} u8 RGB images per call ({H * W * 6 / 1e6:.1f} MB read + written per image)", res,
         "copy_")
    print(f"  R=1: {res['R=1'][0] / res['sharpen R=2'][0]:.2f} x sharpen R=2 (aim: at most 1.5)")
    print(f"  R=2: {res['R=2'][0] / res['chroma R=2'][0]:.2f} x chroma R=2 (aim: at most 1)")
    for r in (1, 2, 3):
        print(f"  R={r}: {res[f'R={r}'][0] / res['sharpen R=2'][0]:.2f} x sharpen R=2, "
              f"{res[f'R={r}'][0] / res['chroma R=1'][0]:.2f} x chroma R=1")
    del srcs, dsts, stack_src, stack_dst

if sys.argv[1:] == ["a"]:
    sys.exit(0)

# (b) what luma_denoise= adds to the ISP's calls
frames = [torch.from_numpy(synthetic.synthetic_packed12(i)).to(dev) for i in range(6)]
SETTINGS = {"off": None, "R=1": ti.LumaDenoise(1), "R=2": ti.LumaDenoise(2), "R=3": ti.LumaDenoise(3)}


def isps(**kw):
    return {name: ti.Camera16(ti.BayerPattern.RGGB, device=dev, luma_denoise=s, **kw) for name, s in SETTINGS.items()}


cams = isps()
images = {name: isp.load_packed12_batch(frames) for name, isp in cams.items()}
show("(b) tonemap_reinhard(write_back=False), six 3072 x 4096 Camera16 images",
     table({n: (lambda n=n: cams[n].tonemap_reinhard(images[n], write_back=False)) for n in cams}, 6), "off")
del images
cams3 = isps(resize_width=1920)
show("(b) config 3: load_packed12_batch(resize_width=1920) + tonemap_reinhard, six frames",
     table({n: (lambda n=n: cams3[n].tonemap_reinhard(cams3[n].load_packed12_batch(frames))) for n in cams3}, 6), "off")
