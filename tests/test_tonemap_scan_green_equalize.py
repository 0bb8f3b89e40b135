"""The scan CLI's --green-equalize options: parsed and checked on the CPU, before any frame is read, and end to end on the
GPU against the library."""
import numpy as np
import pytest

from oracle import isp_oracle as O
from taichi_image_amd.scripts import tonemap_scan as ts
from tests import green_equalize_ref as R
from tests.test_tonemap_scan import _read_png


def test_cli_arguments(tmp_path):
    ap = ts.build_parser()
    a = ap.parse_args(["--images", "x"])
    assert a.green_equalize is False
    assert (a.green_equalize_threshold, a.green_equalize_slope, a.green_equalize_strength, a.green_equalize_radius,
            a.green_equalize_edge) == (None,) * 5
    a = ap.parse_args(["--images", "x", "--green-equalize", "--green-equalize-threshold", "0.01", "--green-equalize-slope",
                       "0.1", "--green-equalize-strength", "0.5", "--green-equalize-radius", "2", "--green-equalize-edge", "3"])
    assert a.green_equalize is True
    assert (a.green_equalize_threshold, a.green_equalize_slope, a.green_equalize_strength, a.green_equalize_radius,
            a.green_equalize_edge) == (0.01, 0.1, 0.5, 2, 3.0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--green-equalize-radius", "1.5"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--green-equalize-threshold"])
    missing = str(tmp_path / "no_such_scan")                                  # (never read: the checks come first)
    for extra in (["--green-equalize-threshold", "0.01"], ["--green-equalize-slope", "0.1"],
                  ["--green-equalize-strength", "0.5"], ["--green-equalize-radius", "2"], ["--green-equalize-edge", "3"]):
        with pytest.raises(ValueError, match="need --green-equalize"):
            ts.main(["--images", missing] + extra)
    for bad in (["--green-equalize-threshold", "-0.01"], ["--green-equalize-threshold", "nan"],
                ["--green-equalize-slope", "inf"], ["--green-equalize-strength", "1.5"],
                ["--green-equalize-radius", "3"], ["--green-equalize-edge", "-1"]):
        with pytest.raises(ValueError, match="GreenEqualize"):
            ts.main(["--images", missing, "--green-equalize"] + bad)
    for good in ([], ["--green-equalize-threshold", "0", "--green-equalize-slope", "0", "--green-equalize-strength", "0",
                      "--green-equalize-radius", "2", "--green-equalize-edge", "0"]):
        with pytest.raises(FileNotFoundError):                                # valid settings get as far as the scan
            ts.main(["--images", missing, "--green-equalize"] + good)


@pytest.mark.gpu
def test_scan_with_green_equalize(tmp_path):
    """One camera x two frames with imbalanced greens: every grid equals the same calls made by hand, and differs from the
    scan without the option."""
    import torch
    import taichi_image_amd as ti
    rng = np.random.default_rng(7)
    H, W = 64, 128
    (tmp_path / "scan" / "cam0").mkdir(parents=True)
    frames = []
    for k in range(2):
        frames.append(O.encode12(R.make_frame(rng, H, W, O.RGGB)))
        (tmp_path / "scan" / "cam0" / f"frame{k}.raw").write_bytes(frames[k].tobytes())
    common = ["--scan", str(tmp_path / "scan"), "--width", str(W), "--rows", "1", "--transform", "none",
              "--moving_alpha", "0.1"]
    out, plain = tmp_path / "out", tmp_path / "plain"
    assert ts.main(common + ["--write", str(out), "--green-equalize", "--green-equalize-radius", "2"]) == 0
    assert ts.main(common + ["--write", str(plain)]) == 0
    dev = torch.device("cuda", 0)
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.1, device=dev, green_equalize=ti.GreenEqualize(radius=2))
    for k in range(2):
        imgs = [isp.load_packed12(torch.from_numpy(frames[k]).to(dev))]
        want = isp.tonemap_reinhard(imgs, gamma=0.9, intensity=3.0, color_adapt=0.0, light_adapt=0.9)
        got = _read_png(out / f"frame{k}.png")
        assert np.array_equal(got, torch.concat(want, dim=1).cpu().numpy()), k
        assert not np.array_equal(got, _read_png(plain / f"frame{k}.png")), k
