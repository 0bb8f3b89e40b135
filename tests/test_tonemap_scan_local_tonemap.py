"""The scan CLI's --local-tonemap options: parsed and checked on the CPU, and end to end on the GPU against the library."""
import numpy as np
import pytest

from taichi_image_amd.scripts import tonemap_scan as ts
from tests.test_tonemap_scan import _read_png
from tests.util import natural_packed12


def test_cli_arguments(tmp_path):
    ap = ts.build_parser()
    a = ap.parse_args(["--images", "x"])
    assert a.local_tonemap is None and a.local_tonemap_floor is None and a.local_tonemap_cell is None
    a = ap.parse_args(["--images", "x", "--local-tonemap", "0.6", "--local-tonemap-floor", "0.002", "--local-tonemap-cell", "16"])
    assert (a.local_tonemap, a.local_tonemap_floor, a.local_tonemap_cell) == (0.6, 0.002, 16)
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--local-tonemap"])
    missing = str(tmp_path / "no_such_scan")                                  # (never read: the checks come first)
    for extra in (["--local-tonemap-floor", "0.002"], ["--local-tonemap-cell", "16"]):
        with pytest.raises(ValueError, match="need --local-tonemap"):
            ts.main(["--images", missing] + extra)
    for bad in (["--local-tonemap", "1.5"], ["--local-tonemap", "nan"], ["--local-tonemap", "0.5", "--local-tonemap-floor", "0"],
                ["--local-tonemap", "0.5", "--local-tonemap-floor", "2"], ["--local-tonemap", "0.5", "--local-tonemap-cell", "12"]):
        with pytest.raises(ValueError, match="LocalTonemap"):
            ts.main(["--images", missing] + bad)
    with pytest.raises(FileNotFoundError):                                    # valid settings get as far as the scan
        ts.main(["--images", missing, "--local-tonemap", "0.5", "--local-tonemap-cell", "64"])


@pytest.mark.gpu
def test_tonemap_scan_with_local_tonemap(tmp_path):
    """Two cameras x two frames: every written grid equals the same calls made by hand, and differs from the scan without
    the stage."""
    import torch
    import taichi_image_amd as ti
    rng = np.random.default_rng(11)
    H, W = 64, 128
    frames = {}
    for cam in ("cam0", "cam1"):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        for k in range(2):
            frames[(cam, k)] = natural_packed12(rng, H, W, dark=0.05)
            (tmp_path / "scan" / cam / f"frame{k}.raw").write_bytes(frames[(cam, k)].tobytes())
    common = ["--scan", str(tmp_path / "scan"), "--width", str(W), "--rows", "1", "--transform", "none", "--moving_alpha", "0.1"]
    out, plain = tmp_path / "out", tmp_path / "plain"
    assert ts.main(common + ["--write", str(out), "--local-tonemap", "0.6", "--local-tonemap-floor", "0.002",
                             "--local-tonemap-cell", "16"]) == 0
    assert ts.main(common + ["--write", str(plain)]) == 0
    dev = torch.device("cuda", 0)
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.1, device=dev,
                      local_tonemap=ti.LocalTonemap(0.6, floor=0.002, cell=16))
    for k in range(2):
        imgs = [isp.load_packed12(torch.from_numpy(frames[(cam, k)]).to(dev)) for cam in ("cam0", "cam1")]
        want = isp.tonemap_reinhard(imgs, gamma=0.9, intensity=3.0, color_adapt=0.0, light_adapt=0.9)
        got = _read_png(out / f"frame{k}.png")
        assert np.array_equal(got, torch.concat(want, dim=1).cpu().numpy()), k
        assert not np.array_equal(got, _read_png(plain / f"frame{k}.png")), k
