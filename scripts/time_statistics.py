"""The cost of the frame statistics: the kernel alone (mi_isp_statistics_raw_batch, six packed 12-bit frames in one call -
the clear and the statistics launch - zones 8 x 8) at 4096 x 3072 and at 1920 x 1440, against its two yardsticks on the same
frames in the same run, the launches alternating round by round: mi_isp_highlights_raw_batch with no clipped pixel (the same
bytes through the same front end, and an f16 CFA written on top: the aim is a time no greater than this one) and a
one-launch device copy of the packed bytes.  Also 32 x 32 zones, and a flat frame (every pixel of a site in one histogram
bin: the worst case of the LDS atomics).  Then load_packed12_batch on the six Camera16 frames with the option off and on,
at both sizes.  HIP-event time per call over 20 calls, the median and the range of seven rounds, in us per frame; bytes
are the packed frame read once (1.5 per pixel)."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
FULL_H, FULL_W = 3072, 4096
ROUNDS, CALLS = 7, 20

SCENES = [np.minimum(np.rint(synthetic.mosaic_rggb(synthetic.synthetic_scene(i, FULL_H, FULL_W)).astype(np.float64) * 4095),
                     int(0.9 * 4095)).astype(np.uint16) for i in range(6)]     # (below the highlights' clip level)


def one_round(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(CALLS): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


def alternating(fns):
    """{name: the sorted times of ROUNDS rounds, us per call}: every round times each of fns once, in turn."""
    for fn in fns.values():
        for _ in range(5): fn()
    times = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            times[name].append(one_round(fn))
    return {name: sorted(t) for name, t in times.items()}


L = _native.lib()
stream = _native.stream_ptr(dev)
hl = ti.Highlights("rebuild", 0.98)._arg((1.8, 1.0, 2.1))
missed = []
for H, W in ((FULL_H, FULL_W), (1440, 1920)):
    nbytes = H * W * 3 // 2
    fr = [torch.from_numpy(synthetic.pack12(np.ascontiguousarray(v12[:H, :W]))).to(dev) for v12 in SCENES]
    flat = [torch.from_numpy(synthetic.pack12(np.full((H, W), 1000, np.uint16))).to(dev)] * 6
    cfas = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in fr]
    copies = torch.empty((6, nbytes), dtype=torch.uint8, device=dev)
    packed = torch.stack([f.reshape(-1) for f in fr])
    s8, s32 = ti.Statistics(zones=(8, 8)), ti.Statistics(zones=(32, 32))
    res8 = torch.empty((6, s8.words), dtype=torch.int64, device=dev)
    res32 = torch.empty((6, s32.words), dtype=torch.int64, device=dev)
    srcs, flats, outs = _native.ptr_array(fr), _native.ptr_array(flat), _native.ptr_array(cfas)
    p8, p32 = _native.ptr_array(list(res8)), _native.ptr_array(list(res32))
    a8, a32 = s8._arg(), s32._arg()
    P12, F16 = _native.MI_RAW_PACKED12, _native.MI_F16
    fns = {
        "statistics 8 x 8": lambda: _native.check(L.mi_isp_statistics_raw_batch(
            srcs, p8, 6, H, W, P12, 0, 0, None, None, a8, stream)),
        "statistics 32 x 32": lambda: _native.check(L.mi_isp_statistics_raw_batch(
            srcs, p32, 6, H, W, P12, 0, 0, None, None, a32, stream)),
        "statistics 8 x 8, flat frame": lambda: _native.check(L.mi_isp_statistics_raw_batch(
            flats, p8, 6, H, W, P12, 0, 0, None, None, a8, stream)),
        "highlights (no clipped pixel)": lambda: _native.check(L.mi_isp_highlights_raw_batch(
            srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, hl, 0, stream)),
        "device copy of the packed bytes": lambda: copies.copy_(packed),
    }
    t = alternating(fns)
    print(f"--- six {W} x {H} packed-12 frames, one call (strips of {L.mi_isp_statistics_strip(6, H, W)} tile(s), "
          f"{L.mi_isp_statistics_direct_blocks(6, H, W, a8)} / {L.mi_isp_statistics_direct_blocks(6, H, W, a32)} blocks per frame "
          f"add to global memory directly at 8 x 8 / 32 x 32 zones)")
    for name, v in t.items():
        med = v[len(v) // 2] / 6
        print(f"kernel alone, {name:32s}: {med:7.2f} us per frame (rounds {v[0] / 6:.2f} .. {v[-1] / 6:.2f}), "
              f"{nbytes / (med * 1e-6) / 1e9:7.1f} GB/s of packed bytes")
    med = {name: v[len(v) // 2] for name, v in t.items()}
    for name in ("statistics 8 x 8", "statistics 32 x 32", "statistics 8 x 8, flat frame"):
        r_hl, r_cp = med[name] / med["highlights (no clipped pixel)"], med[name] / med["device copy of the packed bytes"]
        print(f"{name} / highlights: {r_hl:.3f}    / device copy: {r_cp:.2f}")
        if name == "statistics 8 x 8" and not r_hl <= 1.0:
            missed.append(f"{W} x {H}: {r_hl:.3f}")
    off = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True)
    on = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, statistics=s8)
    t = alternating({"off": lambda: off.load_packed12_batch(fr), "on": lambda: on.load_packed12_batch(fr)})
    a, b = t["off"][ROUNDS // 2] / 6, t["on"][ROUNDS // 2] / 6
    print(f"load_packed12_batch, statistics off: {a:7.2f} us per frame (rounds {t['off'][0] / 6:.2f} .. {t['off'][-1] / 6:.2f})")
    print(f"load_packed12_batch, statistics on : {b:7.2f} us per frame (rounds {t['on'][0] / 6:.2f} .. {t['on'][-1] / 6:.2f}), "
          f"{b - a:+.2f} us, {(b / a - 1) * 100:+.1f} %")
    del fr, flat, cfas, copies, packed
print("the aim (the statistics kernel at 8 x 8 zones takes no more time than the highlights kernel with no clipped pixel on the "
      "same frames): " + ("met at both sizes" if not missed else "MISSED - " + "; ".join(missed)))
