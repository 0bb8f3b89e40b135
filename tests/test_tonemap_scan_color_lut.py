"""The scan CLI's --color-lut / --color-lut-strength: parsed and checked on the CPU, and end to end on the GPU against the
library."""
import numpy as np
import pytest

from taichi_image_amd.scripts import tonemap_scan as ts
from tests import color_lut_ref as C
from tests.test_color_lut_cpu import cube_text
from tests.test_tonemap_scan import _read_png


def test_parser_takes_the_color_lut(tmp_path):
    d = ts.build_parser().parse_args(["--images", "x"])
    assert (d.color_lut, d.color_lut_strength) == (None, None)
    a = ts.build_parser().parse_args(["--images", "x", "--color-lut", "look.cube", "--color-lut-strength", "0.5"])
    assert (str(a.color_lut), a.color_lut_strength) == ("look.cube", 0.5)
    good = tmp_path / "look.cube"
    good.write_text(cube_text(C.look_table(3) / 255.0))
    bad = tmp_path / "bad.cube"
    bad.write_text(cube_text(C.look_table(3) / 255.0).replace("LUT_3D_SIZE 3", "LUT_1D_SIZE 3"))
    for args in (["--color-lut-strength", "0.5"],                   # (no FILE)
                 ["--color-lut", str(bad)],
                 ["--color-lut", str(good), "--color-lut-strength", "1.5"],
                 ["--color-lut", str(good), "--color-lut-strength", "-1"]):
        with pytest.raises(ValueError):                              # refused before any frame is read
            ts.main(["--images", "/nonexistent"] + args)
    with pytest.raises(OSError):
        ts.main(["--images", "/nonexistent", "--color-lut", str(tmp_path / "missing.cube")])


@pytest.mark.gpu
def test_scan_with_a_color_lut(tmp_path):
    """Two cameras x two frames: every grid equals Camera32(color_lut=...) called directly, which is the restatement of the
    plain ISP's output."""
    import torch
    import taichi_image_amd as ti
    from taichi_image_amd import synthetic
    H, W = 64, 128
    frames = {}
    for c, cam in enumerate(("cam0", "cam1")):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        for k in range(2):
            frames[(cam, k)] = synthetic.synthetic_packed12(2 * c + k, H, W)
            (tmp_path / "scan" / cam / f"frame{k}.raw").write_bytes(frames[(cam, k)].tobytes())
    table = C.look_table(9)
    cube = tmp_path / "look.cube"
    cube.write_text(cube_text(table / 255.0))
    out = tmp_path / "out"
    rc = ts.main(["--scan", str(tmp_path / "scan"), "--width", str(W), "--write", str(out), "--rows", "1",
                  "--transform", "none", "--moving_alpha", "0.1", "--color-lut", str(cube), "--color-lut-strength", "0.75"])
    assert rc == 0
    dev = torch.device("cuda", 0)
    plain = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.1, device=dev)
    isp = ti.Camera32(ti.BayerPattern.RGGB, moving_alpha=0.1, device=dev, color_lut=ti.ColorLut(table, 0.75))
    kw = dict(gamma=0.9, intensity=3.0, color_adapt=0.0, light_adapt=0.9)
    for k in range(2):
        want = isp.tonemap_reinhard([isp.load_packed12(torch.from_numpy(frames[(cam, k)]).to(dev)) for cam in ("cam0", "cam1")], **kw)
        base = plain.tonemap_reinhard([plain.load_packed12(torch.from_numpy(frames[(cam, k)]).to(dev)) for cam in ("cam0", "cam1")], **kw)
        got = _read_png(out / f"frame{k}.png")
        assert np.array_equal(got, torch.concat(want, dim=1).cpu().numpy()), k
        ref = np.concatenate([C.color_lut_rgb(b.cpu().numpy(), table, 0.75) for b in base], axis=1)
        assert not np.array_equal(ref, torch.concat(base, dim=1).cpu().numpy())
        assert np.array_equal(got, ref), k
