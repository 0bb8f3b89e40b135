"""The whole-frame kernel (csrc/isp_mega.h) computes two pixels per instruction in its demosaic (pixels K and K + 4 of a
lane) and in its Reinhard map, in the kernels that have the registers for it; the others keep one pixel per instruction.
Every kernel instance - four CFA patterns x color_adapt == 0 / != 0 - on frames with partial bands (height not a multiple
of 12, width not a multiple of 512), with bounds exactly (0, 1) and inside (0, 1), against the C oracle at the parity
contract of tests/util.assert_close; and the same bits from two launches.

The first test needs no GPU: it checks on the oracle alone that the frames are what the GPU cases take them for."""
import numpy as np
import pytest

from oracle import c_oracle, isp_oracle as O
from tests.util import assert_close, assert_exact

pytestmark = pytest.mark.skipif(not c_oracle.available(), reason="oracle/liborc_isp.so not built")

SHAPES = [(26, 520), (130, 1544)]        # 3 / 11 row bands with a partial last one; 2 / 4 column bands, the last 8 / 8 columns wide
KW = [dict(gamma=1.0, intensity=1.0, light_adapt=1.0, color_adapt=0.0),
      dict(gamma=0.6, intensity=1.5, light_adapt=0.7, color_adapt=0.4)]


def frame(H, W, pattern, unit, seed=0):
    """A smooth-plus-noise scene, mosaiced and packed.  unit: two flat patches at code 0 and code 4095, so that the
    demosaiced image's bounds are exactly (0, 1); else the scene is scaled into [0.15, 0.85] and touches neither."""
    rng = np.random.default_rng(1000 * seed + 10 * H + pattern)
    r = np.arange(H)[:, None] / H
    c = np.arange(W)[None, :] / W
    base = 0.1 + 0.8 * (0.5 + 0.5 * np.sin(6.0 * r + 1.0)) * (0.5 + 0.5 * np.cos(9.0 * c))
    img = np.stack([np.clip(base * g + rng.normal(0, 0.03, (H, W)), 0, 1) for g in (1.0, 0.8, 0.6)], -1)
    cfa = O.rgb_to_bayer(img.astype(np.float32), pattern).astype(np.float64)
    if unit:
        cfa[6:12, 8:14] = 0.0
        cfa[H - 12:H - 6, W - 14:W - 8] = 1.0
    else:
        cfa = 0.15 + 0.7 * cfa
    return O.encode12(np.rint(cfa * 4095).astype(np.uint16))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pattern", range(4))
def test_frames_have_the_bounds_the_gpu_cases_assume(shape, pattern):
    H, W = shape
    assert H % 12 != 0 and W % 512 != 0
    for unit in (True, False):
        packed = frame(H, W, pattern, unit)
        cfa = c_oracle.decode12_scaled(packed, work="f16").reshape(H, W)
        rgb = c_oracle.demosaic(cfa, pattern, round_f16=True)
        if unit:
            assert rgb.min() == 0.0 and rgb.max() == 1.0
        else:
            assert rgb.min() > 0.0 and rgb.max() < 1.0
        for kw in KW:
            ref = c_oracle.pipeline12_reinhard(packed, pattern=pattern, work="f16", out="f16", **kw)
            assert ref.shape == (H, W, 3) and np.isfinite(ref.astype(np.float32)).all()
            assert ref.min() == 0.0 and ref.max() == 1.0      # the final map normalises to the mapped image's bounds


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pattern", range(4))
@pytest.mark.parametrize("kw", KW, ids=["ca0", "ca0.4"])
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "nonunit"])
def test_whole_frame_pairs_match_c_oracle_and_repeat(shape, pattern, kw, unit):
    import torch
    import taichi_image_amd as ti
    from taichi_image_amd import _native
    from taichi_image_amd.pipeline import pipeline12_reinhard, whole_frame_fits
    H, W = shape
    dev = torch.device("cuda", 0)
    assert whole_frame_fits(H, W, ti.types.f16)
    packed = frame(H, W, pattern, unit)
    ref = c_oracle.pipeline12_reinhard(packed, pattern=pattern, work="f16", out="f16", **kw)
    src = torch.from_numpy(packed).to(dev)
    outs = []
    for rep in range(2):
        got = pipeline12_reinhard(src, pattern=ti.BayerPattern(pattern), whole_frame=True, **kw)
        torch.cuda.synchronize()
        ws = _native.workspace(H, W, dev)
        off = int(_native.lib().mi_isp_workspace_error_offset(H, W))
        assert int(ws[off:off + 4].view(torch.int32).item()) == 0, "a grid barrier of the whole-frame kernel timed out"
        outs.append(got.cpu().numpy())
    what = f"whole-frame {H}x{W} pattern {pattern} {'unit' if unit else 'non-unit'} bounds {kw}"
    assert_close(outs[0], ref, what)
    assert_exact(outs[1], outs[0], what + ": second launch")
