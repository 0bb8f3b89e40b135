"""The cost of local contrast (CLAHE), median us per image.
(a) The operator alone (mi_isp_local_contrast_rgb_batch, six images per call, outputs and workspace allocated once: four
    launches) on six 3072 x 4096 and six 1440 x 1920 u8 RGB images with 8 x 8 and 16 x 16 tiles, out of place and in
    place, on noise and on a smooth scene (where a wave's pixels share a handful of histogram bins), beside a device-to-device
    copy_ of the same bytes as one launch (the yardstick: the operator reads the image twice and writes it once, 1.5 x the
    copy's bytes) and beside sharpen at radius 1.
(b) What local_contrast= adds per frame to tonemap_reinhard on six full-resolution Camera16 images (write_back=False, so that
    every call sees the same images), to config 3 (load_packed12_batch with resize_width=1920, then tonemap_reinhard) and to
    process_packed12, each against the same call without it.
The variants of one table alternate within every round; a round times each variant over enough calls to fill WINDOW seconds
between two device events, after a warm-up; the figure is the median over the rounds (min .. max beside it).
`python scripts/time_local_contrast.py a` runs part (a) alone (the run to put under a kernel trace)."""
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
        print(f"  {name:16s} {med:8.2f} us per image  ({lo:.2f} .. {hi:.2f}){rel}")


def scene(H, W, seed):
    """A smooth scene with little noise, u8 RGB on the device (the shape of tests/sharpen_ref.scene_u8)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.arange(H, dtype=torch.float32)[:, None] / H
    c = torch.arange(W, dtype=torch.float32)[None, :] / W
    base = 0.1 + 0.8 * (0.5 + 0.5 * torch.sin(6.0 * r + 1.0)) * (0.5 + 0.5 * torch.cos(9.0 * c))
    img = torch.stack([(base * k + 0.01 * torch.randn(H, W, generator=g)).clamp(0, 1) for k in (1.0, 0.8, 0.6)], -1)
    return (img * 255).round().to(torch.uint8).to(dev)


# (a) the operator against a copy
L = _native.lib()
stream = _native.stream_ptr(dev)
g = torch.Generator(device="cpu").manual_seed(1)
for H, W in ((3072, 4096), (1440, 1920)):
    noise = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(6)]
    smooth = [scene(H, W, k) for k in range(6)]
    dsts = [torch.empty_like(s) for s in noise]
    work = [s.clone() for s in smooth]                # (filtered in place again and again: the cost does not depend on it)
    pd = _native.ptr_array(dsts)
    stack_src = torch.stack(noise)                    # the same bytes as one tensor: the copy as ONE launch
    stack_dst = torch.empty_like(stack_src)

    def copy():
        stack_dst.copy_(stack_src)

    def clahe(srcs, outs, lc):
        arg = lc._arg()
        ws = torch.empty(int(L.mi_isp_local_contrast_workspace_bytes(6, arg)), dtype=torch.uint8, device=dev)
        ps, po = _native.ptr_array(srcs), _native.ptr_array(outs)
        return lambda: _native.check(L.mi_isp_local_contrast_rgb_batch(ps, po, 6, H, W, arg, ws.data_ptr(), stream))

    sharp = ti.Sharpen(1.5, 1)._arg()
    pn = _native.ptr_array(noise)
    variants = {"copy_": copy, "sharpen R=1": lambda: _native.check(L.mi_isp_sharpen_rgb_batch(pn, pd, 6, H, W, sharp, stream))}
    for t in (8, 16):
        lc = ti.LocalContrast((t, t))
        variants[f"{t}x{t} noise"] = clahe(noise, dsts, lc)
        variants[f"{t}x{t} scene"] = clahe(smooth, dsts, lc)
        variants[f"{t}x{t} in place"] = clahe(work, work, lc)
    res = table(variants, 6)
    show(f"(a) operator alone, six {H} x {W} u8 RGB images per call ({H * W * 6 / 1e6:.1f} MB read + written per image by the "
         f"copy)", res, "copy_")
    del noise, smooth, dsts, work, stack_src, stack_dst

if sys.argv[1:] == ["a"]:
    sys.exit(0)

# (b) what local_contrast= adds to the ISP's calls
frames = [torch.from_numpy(synthetic.synthetic_packed12(i)).to(dev) for i in range(6)]
SETTINGS = {"off": None, "8x8": ti.LocalContrast((8, 8)), "16x16": ti.LocalContrast((16, 16))}


def isps(**kw):
    return {name: ti.Camera16(ti.BayerPattern.RGGB, device=dev, local_contrast=s, **kw) for name, s in SETTINGS.items()}


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
