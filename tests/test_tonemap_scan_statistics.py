"""The scan CLI's --statistics option: parsed and checked on the CPU, before any frame is read, and end to end on the GPU
against the reference."""
import json

import numpy as np
import pytest

from oracle import isp_oracle as O
from taichi_image_amd.scripts import tonemap_scan as ts
from tests import statistics_ref as R
from tests.test_tonemap_scan import _read_png


def test_cli_arguments(tmp_path):
    ap = ts.build_parser()
    assert ap.parse_args(["--images", "x"]).statistics is None
    assert ap.parse_args(["--images", "x", "--statistics", "4x6"]).statistics == "4x6"
    with pytest.raises(SystemExit):
        ap.parse_args(["--images", "x", "--statistics"])
    missing = str(tmp_path / "no_such_scan")                                  # (never read: the checks come first)
    for bad in ("8", "8x", "x8", "8x8x8", "8.5x8", "+8x8", "axb"):
        with pytest.raises(ValueError, match="--statistics takes GHxGW"):
            ts.main(["--images", missing, "--statistics", bad])
    for bad in ("0x8", "8x33"):
        with pytest.raises(ValueError, match="Statistics.zones"):
            ts.main(["--images", missing, "--statistics", bad])
    for good in ("8x8", "1X32"):
        with pytest.raises(FileNotFoundError):                                # valid settings get as far as the scan
            ts.main(["--images", missing, "--statistics", good])


def test_the_report_writes_nan_as_null():
    class Settings:
        zones, clip, dark = (1, 2), 0.98, 1 / 64

    class Measured:
        def mean(self): return np.array([[[0.5, np.nan, 0.25, 0.125], [0.0] * 4]])
        clipped_fraction = dark_fraction = mean
        def sharpness(self): return np.array([[np.nan, 2.0]])
        def percentile(self, q, site): return np.nan if site == 1 else q / 100

    rep = json.loads(json.dumps(ts.statistics_report(Settings, ["cam0"], [Measured()])))
    cam = rep["cameras"]["cam0"]
    assert rep["zones"] == [1, 2] and cam["mean"][0][0] == [0.5, None, 0.25, 0.125] and cam["sharpness"] == [[None, 2.0]]
    assert cam["percentiles"] == {"1": [0.01, None, 0.01, 0.01], "50": [0.5, None, 0.5, 0.5], "99": [0.99, None, 0.99, 0.99]}


@pytest.mark.gpu
def test_scan_with_statistics(tmp_path):
    """Two cameras x two frames: every <name>.stats.json holds the reference's figures for each camera's frame, and the
    images are those of the scan without the option."""
    rng = np.random.default_rng(7)
    H, W = 64, 128
    frames = {}
    for cam in ("cam0", "cam1"):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        for k in range(2):
            codes = R.make_frame(rng, H, W)
            frames[cam, k] = codes
            (tmp_path / "scan" / cam / f"frame{k}.raw").write_bytes(O.encode12(codes).tobytes())
    common = ["--scan", str(tmp_path / "scan"), "--width", str(W), "--rows", "1", "--transform", "none",
              "--moving_alpha", "0.1"]
    out, plain = tmp_path / "out", tmp_path / "plain"
    assert ts.main(common + ["--write", str(out), "--statistics", "2x4"]) == 0
    assert ts.main(common + ["--write", str(plain)]) == 0
    assert not list(plain.glob("*.json"))
    for k in range(2):
        assert np.array_equal(_read_png(out / f"frame{k}.png"), _read_png(plain / f"frame{k}.png")), k
        rep = json.loads((out / f"frame{k}.stats.json").read_text())
        assert rep["zones"] == [2, 4] and sorted(rep["cameras"]) == ["cam0", "cam1"]
        for cam in ("cam0", "cam1"):
            x = frames[cam, k].astype(np.float32) * np.float32(1 / 4095)
            q = R.measure(x, O.RGGB, (2, 4))
            got = rep["cameras"][cam]
            assert np.array_equal(np.array(got["mean"]), R.mean(q)) and np.array_equal(np.array(got["sharpness"]), R.sharpness(q))
            assert np.array_equal(np.array(got["clipped_fraction"]), R.clipped_fraction(q))
            assert np.array_equal(np.array(got["dark_fraction"]), R.dark_fraction(q))
            assert got["percentiles"] == {str(p): [R.percentile(q, p, s) for s in range(4)] for p in (1, 50, 99)}
