"""The cost of the exposure merge: the kernel alone (mi_isp_merge_raw_batch, one launch for six packed-12 brackets, f16
CFA out) at E = 2 and E = 3, against four reference measurements from the same run - a one-launch device copy of the
bytes the kernel moves (E packed 12-bit frames in, an f16 CFA out: 1.5 E + 2 bytes per pixel), E times the highlight
reconstruction kernel on six frames without a clipped pixel (mi_isp_highlights_raw_batch: the same decode front end per
source frame), the temporal kernel on one frame per camera (mi_isp_temporal_raw_batch), and load_packed12_bracket_batch
against load_packed12_batch of frame 0 alone.  At 4096 x 3072 and at 1920 x 1440.  HIP-event time per call, best of three
rounds of 40 calls after 5 warm-up calls, with the worst round, in us per bracket.

    python scripts/time_exposure_merge.py [out.txt]      (default: profiles/exposure_merge_timing.txt)"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import taichi_image_amd as ti
from taichi_image_amd import _native, synthetic
dev = torch.device("cuda", 0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exposure_merge_timing.txt")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


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
stream = _native.stream_ptr(dev)
GAIN, READ_NOISE = 2.4e-4, 1.5e-3
P12, F16 = _native.MI_RAW_PACKED12, _native.MI_F16
N = 6
for H, W in ((3072, 4096), (1440, 1920)):
    say(f"--- {W} x {H}")
    rng = np.random.default_rng(7)
    scenes = [synthetic.mosaic_rggb(synthetic.synthetic_scene(i, H, W)).astype(np.float64) for i in range(N)]
    cfas = [torch.empty((H, W), dtype=torch.float16, device=dev) for _ in range(N)]
    outs = _native.ptr_array(cfas)

    def exposure(scene, ratio, top):
        """The packed frame of a static scene at `ratio` with model noise, clipped as a sensor does (top: the code)."""
        clean = scene * 0.2 * ratio                      # (a dark scene: the long frames are usable over most of it)
        v = clean + rng.normal(0, 1, clean.shape) * np.sqrt(GAIN * clean + READ_NOISE ** 2)
        return torch.from_numpy(synthetic.pack12(np.clip(np.rint(v * 4095), 0, top).astype(np.uint16))).to(dev)

    # the references: six single frames below the clip level (no clipped pixel)
    single = [exposure(s, 4.5, int(0.9 * 4095)) for s in scenes]
    p_single = _native.ptr_array(single)
    hl_arg = ti.Highlights("rebuild", 0.98)._arg((1.8, 1.0, 2.1))
    tn_arg = ti.TemporalDenoise(GAIN, READ_NOISE)._arg()
    hin = [torch.rand((H, W), dtype=torch.float32, device=dev) for _ in range(N)]
    hout = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(N)]
    p_hin, p_hout = _native.ptr_array(hin), _native.ptr_array(hout)
    hl = timed(lambda: _native.check(L.mi_isp_highlights_raw_batch(
        p_single, outs, N, H, W, P12, 0, F16, 0, None, None, None, hl_arg, 0, stream)))
    tn = timed(lambda: _native.check(L.mi_isp_temporal_raw_batch(
        p_single, p_hin, p_hout, outs, N, H, W, P12, 0, F16, None, None, None, tn_arg, 0, stream)))
    say(f"kernel alone, highlights (no clipped pixel), six frames in one launch: {hl[0] / N:6.2f} us per frame (worst round "
        f"{hl[1] / N:6.2f})")
    say(f"kernel alone, temporal (f16 CFA out)       , six frames in one launch: {tn[0] / N:6.2f} us per frame (worst round "
        f"{tn[1] / N:6.2f})")
    del hin, hout
    off = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True)
    for ratios in ((1, 4), (1, 4, 16)):
        E = len(ratios)
        em = ti.ExposureMerge(ratios, GAIN, READ_NOISE)
        em_arg = em._arg()
        brackets = [[exposure(s, q, 4095) for q in ratios] for s in scenes]
        flat = _native.ptr_array([f for b in brackets for f in b])
        nbytes = H * W * 3 // 2 * E + H * W * 2          # E packed frames in, the f16 CFA out
        k = timed(lambda: _native.check(L.mi_isp_merge_raw_batch(
            flat, outs, N, H, W, P12, 0, F16, None, None, None, em_arg, 0, stream)))
        a = torch.empty(N * nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        cp = timed(lambda: b.copy_(a))
        del a, b
        say(f"E = {E}, ratios {ratios}:")
        say(f"  kernel alone, exposure merge, six brackets in one launch: {k[0] / N:6.2f} us per bracket (worst round "
            f"{k[1] / N:6.2f}), {nbytes / (H * W):5.2f} B per pixel, {nbytes / (k[0] / N * 1e-6) / 1e9:7.1f} GB/s")
        say(f"  a device copy of the same bytes                          : {cp[0] / N:6.2f} us per bracket (worst round "
            f"{cp[1] / N:6.2f}), {nbytes / (cp[0] / N * 1e-6) / 1e9:7.1f} GB/s")
        say(f"  merge / (E x highlights) {k[0] / (E * hl[0]):.2f} (the aim: at most 1), / device copy {k[0] / cp[0]:.2f}, "
            f"/ temporal {k[0] / tn[0]:.2f}")
        on = ti.Camera16(ti.BayerPattern.RGGB, device=dev, correct_colors=True, exposure_merge=em)
        base = timed(lambda: off.load_packed12_batch([b[0] for b in brackets]))
        t = timed(lambda: on.load_packed12_bracket_batch(brackets))
        say(f"  load_packed12_bracket_batch: {t[0] / N:7.2f} us per bracket (worst round {t[1] / N:7.2f}; "
            f"{(t[0] / base[0] - 1) * 100:+.1f} % against load_packed12_batch of frame 0 alone, {base[0] / N:.2f} us per frame)")
        del brackets
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
