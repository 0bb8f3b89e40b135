"""The cost of green equalisation: the kernel alone (mi_isp_green_equalize_raw_batch, six packed 12-bit frames in one launch,
f16 CFA out) at both radii, at 4096 x 3072 and at 1920 x 1440, against its two yardsticks on the same frames in the same
run, the launches alternating round by round: mi_isp_highlights_raw_batch with no clipped pixel (the same front end, a
smaller halo: the floor) and mi_isp_denoise_raw_batch at radius 1 (a weighted same-site window on every site; the aim is a
time no greater than this one at both radii).  Then load_packed12_batch on the six 4096 x 3072 Camera16 frames with the
option off and on.  HIP-event time per call over 20 calls, the median and the range of seven rounds, in us per frame;
bytes are the packed frame read once and the f16 CFA written once (3.5 per pixel)."""
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


def frames(H, W):
    """Six packed H x W frames (the scenes' top-left part), the greens of even rows raised and those of odd rows lowered
    by 2 %."""
    r, c = np.mgrid[0:H, 0:W]
    sign = np.where((r + c) & 1, np.where(r & 1, -1.0, 1.0), 0.0)              # RGGB: green where r + c is odd
    return [torch.from_numpy(synthetic.pack12(np.rint(np.minimum(v12[:H, :W] * (1.0 + 0.02 * sign), 4095)).astype(np.uint16)))
            .to(dev) for v12 in SCENES]


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
ge = {R: ti.GreenEqualize(radius=R)._arg() for R in (1, 2)}
hl = ti.Highlights("rebuild", 0.98)._arg((1.8, 1.0, 2.1))
dn = ti.RawDenoise(0.002, 0.006, radius=1)._arg()
missed = []
for H, W in ((FULL_H, FULL_W), (1440, 1920)):
    nbytes = H * W * 3 // 2 + H * W * 2
    fr = frames(H, W)
    cfas = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in fr]
    plain = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in fr]
    srcs, outs = _native.ptr_array(fr), _native.ptr_array(cfas)
    P12, F16 = _native.MI_RAW_PACKED12, _native.MI_F16
    fns = {
        "green equalize R=1": lambda: _native.check(L.mi_isp_green_equalize_raw_batch(
            srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, ge[1], 0, stream)),
        "green equalize R=2": lambda: _native.check(L.mi_isp_green_equalize_raw_batch(
            srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, ge[2], 0, stream)),
        "highlights (no clipped pixel)": lambda: _native.check(L.mi_isp_highlights_raw_batch(
            srcs, outs, 6, H, W, P12, 0, F16, 0, None, None, None, hl, 0, stream)),
        "denoise R=1": lambda: _native.check(L.mi_isp_denoise_raw_batch(
            srcs, outs, 6, H, W, P12, 0, F16, None, None, None, dn, stream)),
    }
    t = alternating(fns)
    # how much of the frame the correction moves (the gate's pass rate on these scenes)
    _native.check(L.mi_isp_highlights_raw_batch(srcs, _native.ptr_array(plain), 6, H, W, P12, 0, F16, 0, None, None, None, hl,
                                                0, stream))
    fns["green equalize R=1"]()
    torch.cuda.synchronize()
    moved = sum(int((a != b).sum()) for a, b in zip(cfas, plain)) / (3 * H * W)
    print(f"--- six {W} x {H} frames, greens at +-2 %: the correction moves {moved * 100:.1f} % of the green sites at radius 1")
    for name, v in t.items():
        med = v[len(v) // 2] / 6
        print(f"kernel alone, {name:30s}: {med:7.2f} us per frame (rounds {v[0] / 6:.2f} .. {v[-1] / 6:.2f}), "
              f"{nbytes / (med * 1e-6) / 1e9:7.1f} GB/s")
    med = {name: v[len(v) // 2] for name, v in t.items()}
    for R in (1, 2):
        r_hl = med[f"green equalize R={R}"] / med["highlights (no clipped pixel)"]
        r_dn = med[f"green equalize R={R}"] / med["denoise R=1"]
        print(f"green equalize R={R} / highlights: {r_hl:.3f}    green equalize R={R} / denoise R=1: {r_dn:.3f}")
        if not r_dn <= 1.0:
            missed.append(f"{W} x {H} at radius {R}: {r_dn:.3f}")
    if (H, W) == (FULL_H, FULL_W):
        off = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True)
        on = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, green_equalize=ti.GreenEqualize())
        t = alternating({"off": lambda: off.load_packed12_batch(fr), "on": lambda: on.load_packed12_batch(fr)})
        a, b = t["off"][ROUNDS // 2] / 6, t["on"][ROUNDS // 2] / 6
        print(f"load_packed12_batch, green equalize off: {a:7.2f} us per frame (rounds {t['off'][0] / 6:.2f} .. {t['off'][-1] / 6:.2f})")
        print(f"load_packed12_batch, green equalize on : {b:7.2f} us per frame (rounds {t['on'][0] / 6:.2f} .. {t['on'][-1] / 6:.2f}), "
              f"{b - a:+.2f} us, {(b / a - 1) * 100:+.1f} %")
    del fr, cfas, plain
print("the aim (the green equalize kernel at both radii takes no more time than the denoise kernel at radius 1 on the same "
      "frames): " + ("met in every case" if not missed else "MISSED - " + "; ".join(missed)))
