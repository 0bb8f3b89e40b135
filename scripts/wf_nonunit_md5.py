"""md5 sums of the whole-frame kernel's outputs on two 4K frames whose bounds are not (0, 1) (the frames of
scripts/wf_nonunit.py: code * 0.7 + 0.1 * 4095), under several parameter sets - for comparing two builds bit for bit.
    [MI_ISP_LIB=...] python scripts/wf_nonunit_md5.py"""
import hashlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taichi_image_amd import _native, synthetic, types
from taichi_image_amd.pipeline import pipeline12_reinhard
H, W = 3072, 4096
dev = torch.device("cuda", 0)
def rescale(p):
    b = p.reshape(H, -1, 3).astype(np.uint32)
    v = np.stack([b[..., 0] | ((b[..., 1] & 0xF) << 8), (b[..., 1] >> 4) | (b[..., 2] << 4)], -1).reshape(H, W)
    return synthetic.pack12(np.rint(v * 0.7 + 0.1 * 4095).astype(np.uint16))
SETS = [{}, dict(gamma=0.6, intensity=1.5, light_adapt=0.7), dict(gamma=0.6, intensity=1.5, light_adapt=0.7, color_adapt=0.4),
        dict(dtype=types.u8)]
off = int(_native.lib().mi_isp_workspace_error_offset(H, W))
for k in range(2):
    frame = torch.from_numpy(rescale(synthetic.synthetic_packed12(k))).to(dev)
    for kw in SETS:
        out = pipeline12_reinhard(frame, whole_frame=True, **kw)
        torch.cuda.synchronize()
        err = int(_native.workspace(H, W, dev)[off:off + 4].view(torch.int32).item())
        what = sorted((n, "u8" if n == "dtype" else str(v)) for n, v in kw.items())
        print(f"nonunit frame {k} {what} {hashlib.md5(out.cpu().numpy().tobytes()).hexdigest()} fault word {err}", flush=True)
