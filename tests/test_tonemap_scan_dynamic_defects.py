"""The scan CLI's --dynamic-defects options: parsed and checked on the CPU, before any frame is read, and end to end on the
GPU against the library."""
import numpy as np
import pytest

from taichi_image_amd.scripts import tonemap_scan as ts
from tests import dynamic_defects_ref as R
from tests.test_tonemap_scan import _read_png


def test_cli_arguments(tmp_path):
    ap = ts.build_parser()
    a = ap.parse_args(["--images", "x"])
    assert a.dynamic_defects is False and a.dynamic_defects_threshold is None and a.dynamic_defects_slope is None
    assert a.dynamic_defects_tolerate is None
    a = ap.parse_args(["--images", "x", "--dynamic-defects", "--dynamic-defects-threshold", "0.03",
                       "--dynamic-defects-slope", "0.25", "--dynamic-defects-tolerate", "0"])
    assert a.dynamic_defects is True
    assert (a.dynamic_defects_threshold, a.dynamic_defects_slope, a.dynamic_defects_tolerate) == (0.03, 0.25, 0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--dynamic-defects-tolerate", "0.5"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--dynamic-defects-threshold"])
    missing = str(tmp_path / "no_such_scan")                                  # (never read: the checks come first)
    for extra in (["--dynamic-defects-threshold", "0.03"], ["--dynamic-defects-slope", "0.25"],
                  ["--dynamic-defects-tolerate", "1"]):
        with pytest.raises(ValueError, match="need --dynamic-defects"):
            ts.main(["--images", missing] + extra)
    for bad in (["--dynamic-defects-threshold", "0"], ["--dynamic-defects-threshold", "nan"],
                ["--dynamic-defects-threshold", "-0.02"], ["--dynamic-defects-slope", "-1"],
                ["--dynamic-defects-slope", "inf"], ["--dynamic-defects-tolerate", "2"]):
        with pytest.raises(ValueError, match="DynamicDefects"):
            ts.main(["--images", missing, "--dynamic-defects"] + bad)
    for good in ([], ["--dynamic-defects-threshold", "0.03", "--dynamic-defects-slope", "0", "--dynamic-defects-tolerate", "0"]):
        with pytest.raises(FileNotFoundError):                                # valid settings get as far as the scan
            ts.main(["--images", missing, "--dynamic-defects"] + good)


@pytest.mark.gpu
def test_scan_with_dynamic_defects(tmp_path):
    """One camera x two frames with injected defects: every grid equals the same calls made by hand, and differs from the
    scan without the option."""
    import torch
    import taichi_image_amd as ti
    from oracle import isp_oracle as O
    rng = np.random.default_rng(7)
    H, W = 64, 128
    (tmp_path / "scan" / "cam0").mkdir(parents=True)
    frames = []
    for k in range(2):
        codes, _ = R.make_frame(rng, H, W)
        frames.append(O.encode12(codes))
        (tmp_path / "scan" / "cam0" / f"frame{k}.raw").write_bytes(frames[k].tobytes())
    common = ["--scan", str(tmp_path / "scan"), "--width", str(W), "--rows", "1", "--transform", "none",
              "--moving_alpha", "0.1"]
    out, plain = tmp_path / "out", tmp_path / "plain"
    assert ts.main(common + ["--write", str(out), "--dynamic-defects", "--dynamic-defects-tolerate", "0"]) == 0
    assert ts.main(common + ["--write", str(plain)]) == 0
    dev = torch.device("cuda", 0)
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.1, device=dev, dynamic_defects=ti.DynamicDefects(tolerate=0))
    for k in range(2):
        imgs = [isp.load_packed12(torch.from_numpy(frames[k]).to(dev))]
        want = isp.tonemap_reinhard(imgs, gamma=0.9, intensity=3.0, color_adapt=0.0, light_adapt=0.9)
        got = _read_png(out / f"frame{k}.png")
        assert np.array_equal(got, torch.concat(want, dim=1).cpu().numpy()), k
        assert not np.array_equal(got, _read_png(plain / f"frame{k}.png")), k
