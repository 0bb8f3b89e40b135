"""The scan CLI's --auto-white-balance: parsed on the CPU, and end to end on the GPU against the library."""
import numpy as np
import pytest

from taichi_image_amd.scripts import tonemap_scan as ts
from tests.test_tonemap_scan import _read_png


def test_parser_takes_auto_white_balance():
    assert ts.build_parser().parse_args(["--images", "x"]).auto_white_balance is False
    assert ts.build_parser().parse_args(["--images", "x", "--auto-white-balance"]).auto_white_balance is True


@pytest.mark.gpu
def test_scan_with_auto_white_balance(tmp_path):
    """Two cameras x three frames: every grid equals Camera32(auto_white_balance=True) called directly, and the loop
    moved the gains away from the seed."""
    import torch
    import taichi_image_amd as ti
    from taichi_image_amd import synthetic
    H, W = 64, 128
    frames = {}
    for c, cam in enumerate(("cam0", "cam1")):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        for k in range(3):
            frames[(cam, k)] = synthetic.synthetic_packed12(3 * c + k, H, W)
            (tmp_path / "scan" / cam / f"frame{k}.raw").write_bytes(frames[(cam, k)].tobytes())
    out = tmp_path / "out"
    rc = ts.main(["--scan", str(tmp_path / "scan"), "--width", str(W), "--write", str(out), "--rows", "1",
                  "--transform", "none", "--moving_alpha", "0.1", "--auto-white-balance"])
    assert rc == 0
    dev = torch.device("cuda", 0)
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.1, device=dev, auto_white_balance=True)
    for k in range(3):
        imgs = [isp.load_packed12(torch.from_numpy(frames[(cam, k)]).to(dev)) for cam in ("cam0", "cam1")]
        want = isp.tonemap_reinhard(imgs, gamma=0.9, intensity=3.0, color_adapt=0.0, light_adapt=0.9)
        assert np.array_equal(_read_png(out / f"frame{k}.png"), torch.concat(want, dim=1).cpu().numpy()), k
    assert not np.array_equal(isp.white_balance_gains.cpu().numpy(), np.array([1.8, 1.0, 2.1], np.float32))
