"""The whole-frame kernel (csrc/isp_mega.h) does the scalar-free half of phase C's work on its five LDS rows - read,
conversions, normalisation, gray, smallest and largest channel - inside the wait of barrier 0, assuming bounds (0, 1), and
again inside barrier 1's wait when the bounds turn out otherwise.  What can go wrong with that: a last row band that ends
inside the LDS rows (rows 0..4 of a band of 12) or just behind them, values of the previous frame of a batch, or of the
speculative pass, taken for this frame's, and a kernel instance that was not meant to change (color_adapt != 0).

Reference: the C oracle at the parity contract of tests/util.assert_close; for the batches, the frame's own single launch,
bit for bit.  Every GPU test asserts that the workspace's fault word is 0.

The first test needs no GPU: it checks on the oracle alone that the frames have the bounds the GPU cases take them for."""
import numpy as np
import pytest

from oracle import c_oracle, isp_oracle as O
from tests.util import assert_close

pytestmark = pytest.mark.skipif(not c_oracle.available(), reason="oracle/liborc_isp.so not built")

# H mod 12 in {2, 4}: the last band ends inside the LDS rows; in {6, 10}: just behind them / inside the register rows.
# Widths: one band, a band and 8 columns, two bands and 8 columns.
SHAPES_INSIDE = [(14, 520), (28, 512), (4, 8)]
SHAPES_BEHIND = [(18, 1032), (34, 520)]
SHAPES_OTHER = [(12, 8), (64, 512)]                     # a single active lane (one band of 12 rows); 5 full bands + 4 rows


def frame(H, W, pattern, unit, seed=0):
    """A smooth-plus-noise scene, mosaiced and packed.  unit: flat 6 x 6 patches at code 0 (top left) and code 4095 (bottom
    right), so that the demosaiced image's bounds are exactly (0, 1) - frames of 12 rows or more; else the scene is scaled
    into [0.1, 0.8] (gain 0.7, offset 0.1) and touches neither."""
    rng = np.random.default_rng(1000 * seed + 10 * H + pattern)
    r = np.arange(H)[:, None] / H
    c = np.arange(W)[None, :] / W
    base = 0.1 + 0.8 * (0.5 + 0.5 * np.sin(6.0 * r + 1.0)) * (0.5 + 0.5 * np.cos(9.0 * c))
    img = np.stack([np.clip(base * g + rng.normal(0, 0.03, (H, W)), 0, 1) for g in (1.0, 0.8, 0.6)], -1)
    cfa = O.rgb_to_bayer(img.astype(np.float32), pattern).astype(np.float64)
    if unit:
        assert H >= 12 and W >= 8
        cfa[0:6, 0:6] = 0.0
        cfa[H - 6:H, W - 6:W] = 1.0
    else:
        cfa = 0.1 + 0.7 * cfa
    return O.encode12(np.rint(cfa * 4095).astype(np.uint16))


def cases(shapes):
    return [(s, unit) for s in shapes for unit in (True, False) if not (unit and s[0] < 12)]


def case_id(c):
    return f"{c[0][0]}x{c[0][1]}-{'unit' if c[1] else 'nonunit'}"


ALL_CASES = cases(SHAPES_INSIDE + SHAPES_BEHIND + SHAPES_OTHER + [(28, 1032), (26, 520)])


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_frames_have_the_bounds_the_gpu_cases_assume(case):
    (H, W), unit = case
    assert H % 2 == 0 and W % 2 == 0
    # (28, 1032) is the shape of the CFA pattern cases, (26, 520) that of the batches (one seed per frame)
    for pattern, seed in [(p, 0) for p in (range(4) if (H, W) == (28, 1032) else (0,))] + [(0, k) for k in range(1, 6) if (H, W) == (26, 520)]:
        packed = frame(H, W, pattern, unit, seed)
        cfa = c_oracle.decode12_scaled(packed, work="f16").reshape(H, W)
        rgb = c_oracle.demosaic(cfa, pattern, round_f16=True)
        if unit:
            assert rgb.min() == 0.0 and rgb.max() == 1.0
        else:
            assert rgb.min() > 0.0 and rgb.max() < 1.0


def run_single(packed, pattern=0, out="f16", **kw):
    """One launch of the whole-frame kernel; its fault word must be 0."""
    import torch
    import taichi_image_amd as ti
    from taichi_image_amd import _native
    from taichi_image_amd.pipeline import pipeline12_reinhard, whole_frame_fits
    H, W = packed.shape[0], packed.shape[1] * 2 // 3
    dev = torch.device("cuda", 0)
    dt = getattr(ti.types, out)
    assert whole_frame_fits(H, W, dt)
    got = pipeline12_reinhard(torch.from_numpy(packed).to(dev), pattern=ti.BayerPattern(pattern), dtype=dt, whole_frame=True, **kw)
    torch.cuda.synchronize()
    ws = _native.workspace(H, W, dev)
    off = int(_native.lib().mi_isp_workspace_error_offset(H, W))
    assert int(ws[off:off + 4].view(torch.int32).item()) == 0, "a grid barrier of the whole-frame kernel timed out"
    return got


def check_against_oracle(shape, unit, pattern=0, out="f16", **kw):
    H, W = shape
    packed = frame(H, W, pattern, unit)
    ref = c_oracle.pipeline12_reinhard(packed, pattern=pattern, work="f16", out=out, **kw)
    got = run_single(packed, pattern, out, **kw).cpu().numpy()
    assert_close(got, ref, f"whole-frame {H}x{W} pattern {pattern} {'unit' if unit else 'non-unit'} bounds, {out} {kw}")


@pytest.mark.gpu
@pytest.mark.parametrize("out", ["f16", "u8"])
@pytest.mark.parametrize("case", cases(SHAPES_INSIDE), ids=case_id)
def test_last_band_ends_inside_the_lds_rows(case, out):
    assert case[0][0] % 12 in (2, 4)
    check_against_oracle(case[0], case[1], out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("out", ["f16", "u8"])
@pytest.mark.parametrize("case", cases(SHAPES_BEHIND), ids=case_id)
def test_last_band_ends_behind_the_lds_rows(case, out):
    assert case[0][0] % 12 in (6, 10)
    check_against_oracle(case[0], case[1], out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "nonunit"])
@pytest.mark.parametrize("pattern", range(4))
def test_all_cfa_patterns(pattern, unit):
    check_against_oracle((28, 1032), unit, pattern=pattern)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "nonunit"])
def test_color_adapt_takes_the_rgb_kernel_unchanged(unit):
    check_against_oracle((26, 520), unit, gamma=0.6, intensity=1.5, light_adapt=0.7, color_adapt=0.4)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(SHAPES_OTHER), ids=case_id)
def test_single_lane_band_and_full_bands(case):
    check_against_oracle(case[0], case[1])


@pytest.mark.gpu
@pytest.mark.parametrize("first_unit", [True, False], ids=["unit_first", "nonunit_first"])
def test_batch_of_alternating_bounds_takes_no_stale_ahead_values(first_unit):
    """Six frames in ONE launch, bounds (0, 1) and not, alternating: the values computed ahead for a frame under the
    assumption of unit bounds, and those of the frame before, must not reach a frame they do not belong to."""
    import torch
    import taichi_image_amd as ti
    from taichi_image_amd import _native
    from taichi_image_amd.pipeline import BatchPipeline
    H, W, n = 26, 520, 6
    dev = torch.device("cuda", 0)
    host = [frame(H, W, 0, (k % 2 == 0) == first_unit, seed=k) for k in range(n)]
    single = [run_single(h).cpu() for h in host]
    bp = BatchPipeline(n, H, W, dev, whole_frame=True)
    outs = bp([torch.from_numpy(h).to(dev) for h in host])
    torch.cuda.synchronize()
    off = int(_native.lib().mi_isp_workspace_error_offset(H, W))
    wsb = bp.ws.numel() // n
    for k in range(n):
        assert int(bp.ws[k * wsb + off:k * wsb + off + 4].view(torch.int32).item()) == 0, f"frame {k}: a grid barrier timed out"
    for k in range(n):
        assert outs[k].dtype == torch.float16 and single[k].dtype == torch.float16
        assert torch.equal(outs[k].cpu().view(torch.int16), single[k].view(torch.int16)), \
            f"frame {k} of the batch ({'unit' if (k % 2 == 0) == first_unit else 'non-unit'} bounds) differs from its own single launch"
    # and the single launches are the oracle's frames
    for k in (0, 1):
        assert_close(single[k].numpy(), c_oracle.pipeline12_reinhard(host[k], pattern=0, work="f16", out="f16"), f"single launch {k}")
