"""The scan CLI's --temporal-denoise options: parsed and checked on the CPU, and end to end on the GPU against the
library (one history per camera folder, kept across the scan's frames)."""
import numpy as np
import pytest

from taichi_image_amd.scripts import tonemap_scan as ts
from tests import temporal_ref as T
from tests.test_tonemap_scan import _read_png

GAIN, READ_NOISE = 2.4e-4, 1.5e-3


def test_cli_arguments(tmp_path):
    ap = ts.build_parser()
    a = ap.parse_args(["--images", "x"])
    assert a.temporal_denoise is None and a.temporal_threshold is None and a.temporal_max_weight is None
    a = ap.parse_args(["--images", "x", "--temporal-denoise", "2.4e-4", "1.5e-3", "--temporal-threshold", "2.5",
                       "--temporal-max-weight", "0.5", "--reverse"])
    assert a.temporal_denoise == [2.4e-4, 1.5e-3] and a.temporal_threshold == 2.5 and a.temporal_max_weight == 0.5
    assert a.reverse is True                                                  # (allowed: it is still a sequence)
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--temporal-denoise", "2.4e-4"])
    missing = str(tmp_path / "no_such_scan")                                  # (never read: the checks come first)
    for extra in (["--temporal-threshold", "2.5"], ["--temporal-max-weight", "0.5"]):
        with pytest.raises(ValueError, match="need --temporal-denoise"):
            ts.main(["--images", missing] + extra)
    for bad in (["--temporal-denoise", "-1", "1.5e-3"], ["--temporal-denoise", "2.4e-4", "0"],
                ["--temporal-denoise", "2.4e-4", "nan"],
                ["--temporal-denoise", "2.4e-4", "1.5e-3", "--temporal-threshold", "0"],
                ["--temporal-denoise", "2.4e-4", "1.5e-3", "--temporal-max-weight", "1"],
                ["--temporal-denoise", "2.4e-4", "1.5e-3", "--temporal-max-weight", "inf"]):
        with pytest.raises(ValueError, match="TemporalDenoise"):
            ts.main(["--images", missing] + bad)
    with pytest.raises(FileNotFoundError):                                    # valid settings get as far as the scan
        ts.main(["--images", missing, "--temporal-denoise", "2.4e-4", "1.5e-3", "--temporal-max-weight", "0.5", "--reverse"])


@pytest.mark.gpu
def test_scan_with_temporal_denoise(tmp_path):
    """Two cameras x three frames of a noisy static scene with a moving quarter: every grid equals the same calls made by
    hand with one TemporalHistory per camera, and from the second frame on differs from the scan without the stage."""
    import torch
    import taichi_image_amd as ti
    from oracle import isp_oracle as O
    rng = np.random.default_rng(7)
    H, W = 64, 128
    frames = {}
    for cam in ("cam0", "cam1"):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        for k, u in enumerate(T.make_sequence(rng, H, W, 3, GAIN, READ_NOISE)):
            frames[(cam, k)] = O.encode12(np.rint(u * 4095).astype(np.uint16))
            (tmp_path / "scan" / cam / f"frame{k}.raw").write_bytes(frames[(cam, k)].tobytes())
    common = ["--scan", str(tmp_path / "scan"), "--width", str(W), "--rows", "1", "--transform", "none",
              "--moving_alpha", "0.1"]
    out, plain = tmp_path / "out", tmp_path / "plain"
    assert ts.main(common + ["--write", str(out), "--temporal-denoise", str(GAIN), str(READ_NOISE),
                             "--temporal-threshold", "2.5", "--temporal-max-weight", "0.6"]) == 0
    assert ts.main(common + ["--write", str(plain)]) == 0
    dev = torch.device("cuda", 0)
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.1, device=dev,
                      temporal_denoise=ti.TemporalDenoise(GAIN, READ_NOISE, threshold=2.5, max_weight=0.6))
    hists = {cam: ti.TemporalHistory() for cam in ("cam0", "cam1")}
    for k in range(3):
        imgs = [isp.load_packed12(torch.from_numpy(frames[(cam, k)]).to(dev), history=hists[cam]) for cam in ("cam0", "cam1")]
        want = isp.tonemap_reinhard(imgs, gamma=0.9, intensity=3.0, color_adapt=0.0, light_adapt=0.9)
        got = _read_png(out / f"frame{k}.png")
        assert np.array_equal(got, torch.concat(want, dim=1).cpu().numpy()), k
        assert np.array_equal(got, _read_png(plain / f"frame{k}.png")) == (k == 0), k
    assert all(h.frames == 3 for h in hists.values())
