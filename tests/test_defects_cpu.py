"""Defective pixel correction without a GPU: DefectMap, the contract of DESIGN.md 3 restated in NumPy on hand-derived
vectors, find_defects, the output lists of the packed fix-up, the C entry points' host checks and the scan CLI's
--defect-pixels validation."""
import ctypes

import numpy as np
import pytest

from oracle import isp_oracle as O
from taichi_image_amd import defects as D
from taichi_image_amd.defects import DefectMap, find_defects

f32 = np.float32
AXIAL = [(-2, 0), (2, 0), (0, -2), (0, 2)]
DIAGONAL = [(-2, -2), (-2, 2), (2, -2), (2, 2)]


def correct_cfa(x, mask, work):
    """The contract: x the (H, W) work-dtype CFA the loader gives (any float dtype holding work-dtype values), mask the
    defect mask.  Returns the corrected CFA in the work dtype: every listed site the f32 mean, in list order, of its
    kept axial neighbours at distance 2 (the diagonals when none is kept), cast by O.cast_out; no kept one: x itself."""
    xf = np.asarray(x).astype(f32)
    H, W = xf.shape
    y = O.cast_out(xf, work)
    for r, c in np.argwhere(mask):
        for cand in (AXIAL, DIAGONAL):
            kept = [xf[r + dr, c + dc] for dr, dc in cand
                    if 0 <= r + dr < H and 0 <= c + dc < W and not mask[r + dr, c + dc]]
            if kept:
                break
        if not kept:
            continue
        s = kept[0]
        for v in kept[1:]:
            s = f32(s + v)
        y[r, c] = O.cast_out(np.array([f32(s) / f32(len(kept))], f32), work)[0]
    return y


def _mask(H, W, sites):
    m = np.zeros((H, W), bool)
    for r, c in sites:
        m[r, c] = True
    return m


# ---- DefectMap --------------------------------------------------------------------------------------------------------
def test_defect_map_validation_dedupe_and_sort():
    m = DefectMap([[5, 3], [0, 1], [5, 3], [2, 7]], (8, 10))
    assert m.coords.tolist() == [[0, 1], [2, 7], [5, 3]] and m.coords.dtype == np.int32
    assert len(m) == 3 and m.shape == (8, 10)
    assert len(DefectMap(np.zeros((0, 2), np.int64), (4, 4))) == 0
    assert len(DefectMap([], (4, 4))) == 0
    for coords, shape in (([[0, 10]], (8, 10)), ([[8, 0]], (8, 10)), ([[-1, 0]], (8, 10)), ([[0.5, 1]], (8, 10)),
                          ([[True, False]], (8, 10)), ([[1, 2, 3]], (8, 10)), ([1, 2], (8, 10)), ([[0, 0]], (7, 10)),
                          ([[0, 0]], (8, 9)), ([[0, 0]], (0, 10)), ([[0, 0]], (8,)), ([[0, 0]], (8.0, 10))):
        with pytest.raises(ValueError):
            DefectMap(coords, shape)


def test_from_mask_round_trip(rng):
    mask = rng.random((12, 18)) < 0.1
    m = DefectMap.from_mask(mask)
    assert np.array_equal(m.mask(), mask) and m.shape == (12, 18)
    assert np.array_equal(DefectMap(m.coords[::-1], m.shape).coords, m.coords)
    words = m.mask_words()
    assert words.shape == (12, 1)
    bits = (words[:, :, None] >> np.arange(32)) & 1
    assert np.array_equal(bits.reshape(12, 32)[:, :18].astype(bool), mask)
    with pytest.raises(ValueError):
        DefectMap.from_mask(mask.astype(np.uint8))


def test_check_defects():
    m = DefectMap([[1, 1]], (8, 10))
    assert D.check_defects(None, (8, 10)) is None
    assert D.check_defects(DefectMap([], (8, 10)), (8, 10)) is None
    assert D.check_defects(m, (8, 10)) is m
    with pytest.raises(ValueError):
        D.check_defects(m, (8, 12))
    with pytest.raises(ValueError):
        D.check_defects(np.array([[1, 1]]), (8, 10))


# ---- the contract on hand-derived vectors -------------------------------------------------------------------------------
def test_isolated_defect_is_the_mean_of_four():
    x = np.zeros((8, 8), f32)
    x[2, 4], x[6, 4], x[4, 2], x[4, 6] = 0.25, 0.5, 0.75, 1.0
    x[4, 4] = 1000.0
    y = correct_cfa(x, _mask(8, 8, [(4, 4)]), "f32")
    assert y[4, 4] == f32(0.625)
    assert np.array_equal(np.delete(y.reshape(-1), 4 * 8 + 4), np.delete(x.reshape(-1), 4 * 8 + 4))


def test_edge_defect_takes_three_with_a_rounded_division():
    x = np.zeros((8, 8), f32)
    x[0, 0], x[4, 0], x[2, 2] = 0.1, 0.1, 0.1        # (2, 0): up (0, 0), down (4, 0), right (2, 2); left is outside
    y = correct_cfa(x, _mask(8, 8, [(2, 0)]), "f32")
    s = f32(f32(f32(0.1) + f32(0.1)) + f32(0.1))
    assert y[2, 0] == f32(s / f32(3))
    assert f32(s / f32(3)) != f32(s * f32(1.0 / 3.0))                  # a correctly rounded division, not s * rcp(3)


def test_corner_defect_takes_two():
    x = np.zeros((6, 6), f32)
    x[2, 0], x[0, 2] = 0.5, 0.25
    y = correct_cfa(x, _mask(6, 6, [(0, 0)]), "f32")
    assert y[0, 0] == f32(0.375)
    y = correct_cfa(x, _mask(6, 6, [(5, 5)]), "f32")                # (3, 5) and (5, 3)
    assert y[5, 5] == f32(0.0)


def test_axial_neighbours_all_defective_take_the_diagonals():
    x = np.arange(100, dtype=f32).reshape(10, 10) / f32(100)
    sites = [(4, 4), (2, 4), (6, 4), (4, 2), (4, 6)]
    y = correct_cfa(x, _mask(10, 10, sites), "f32")
    diag = [x[2, 2], x[2, 6], x[6, 2], x[6, 6]]
    assert y[4, 4] == f32(f32(f32(f32(diag[0] + diag[1]) + diag[2]) + diag[3]) / f32(4))
    # (2, 4): up (0, 4), left (2, 2) and right (2, 6) kept, down (4, 4) defective
    assert y[2, 4] == f32(f32(f32(x[0, 4] + x[2, 2]) + x[2, 6]) / f32(3))


def test_fully_surrounded_site_is_kept():
    x = np.random.default_rng(3).random((10, 10)).astype(f32)
    sites = [(4, 4)] + [(4 + dr, 4 + dc) for dr, dc in AXIAL + DIAGONAL]
    y = correct_cfa(x, _mask(10, 10, sites), "f32")
    assert y[4, 4] == x[4, 4]
    # one colour entirely defective: every site keeps its value (the n = 0 rule)
    every = [(r, c) for r in range(0, 10, 2) for c in range(1, 10, 2)]
    assert np.array_equal(correct_cfa(x, _mask(10, 10, every), "f32"), x)


def test_mean_is_rounded_to_f16():
    x = np.zeros((6, 6), np.float16)
    x[0, 2], x[4, 2], x[2, 0], x[2, 4] = np.float16(0.1), np.float16(0.2), np.float16(0.3), np.float16(0.7)
    y = correct_cfa(x, _mask(6, 6, [(2, 2)]), "f16")
    xs = x.astype(f32)
    s = f32(f32(f32(xs[0, 2] + xs[4, 2]) + xs[2, 0]) + xs[2, 4])
    assert y.dtype == np.float16 and y[2, 2] == np.float16(s / f32(4))
    assert f32(y[2, 2]) != s / f32(4)                                  # the f32 mean is not an f16 value


# ---- output lists of the packed fix-up -----------------------------------------------------------------------------------
def _reads(H, W, Hd, Wd, scale, mask):
    """Brute force: the output pixels whose value reads a defective site (through the 13-tap diamond, the bilinear taps)."""
    dia = np.zeros((H, W), bool)
    for r, c in np.argwhere(mask):
        for dr, dc in O.DIAMOND:
            if 0 <= r + dr < H and 0 <= c + dc < W:
                dia[r + dr, c + dc] = True
    if not scale > 0:
        return dia
    s = f32(scale)
    out = np.zeros((Hd, Wd), bool)
    for i in range(Hd):
        pr = f32(i) / s
        r0, r1 = min(int(pr), H - 1), min(int(pr) + 1, H - 1)
        for j in range(Wd):
            pc = f32(j) / s
            c0, c1 = min(int(pc), W - 1), min(int(pc) + 1, W - 1)
            out[i, j] = dia[r0, c0] or dia[r1, c0] or dia[r0, c1] or dia[r1, c1]
    return out


@pytest.mark.parametrize("Hd,Wd,scale", [(34, 46, 0.0), (17, 23, 0.5), (16, 21, 0.46875), (68, 92, 2.0), (25, 34, 0.75)])
def test_affected_outputs_cover_every_reader(rng, Hd, Wd, scale):
    H, W = 34, 46
    mask = rng.random((H, W)) < 0.02
    mask[0, 0] = mask[H - 1, W - 1] = mask[0, W - 1] = True
    m = DefectMap.from_mask(mask)
    lst = m.affected_outputs(Hd, Wd, scale)
    assert lst.dtype == np.int32 and np.all(np.diff(lst) > 0)                       # sorted and unique
    listed = np.zeros(Hd * Wd, bool)
    listed[lst] = True
    need = _reads(H, W, Hd, Wd, scale, mask).reshape(-1)
    assert not (need & ~listed).any(), "an output that reads a defective site is not listed"
    assert len(DefectMap([], (H, W)).affected_outputs(Hd, Wd, scale)) == 0


# ---- find_defects -------------------------------------------------------------------------------------------------------
def test_find_defects_recovers_hot_and_dead_pixels():
    rng = np.random.default_rng(11)
    H, W, K = 48, 64, 8
    hot = [(0, 0), (0, 63), (47, 0), (47, 63), (0, 30), (23, 0), (20, 33), (31, 17), (1, 62)]
    dark = rng.normal(64, 3, (K, H, W))
    for r, c in hot:
        dark[:, r, c] += 400
    got = find_defects(np.clip(np.rint(dark), 0, 4095).astype(np.uint16), threshold=40)
    assert sorted(map(tuple, got.coords.tolist())) == sorted(hot) and got.shape == (H, W)
    dead = [(0, 1), (47, 62), (10, 10), (11, 11), (30, 0), (2, 63)]
    flat = rng.normal(3000, 20, (K, H, W))
    for r, c in dead:
        flat[:, r, c] = rng.normal(5, 2, K)
    got = find_defects(np.clip(np.rint(flat), 0, 4095).astype(np.uint16), threshold=400)
    assert sorted(map(tuple, got.coords.tolist())) == sorted(dead)
    with pytest.raises(ValueError):
        find_defects(np.zeros((2, 3)), 1.0)
    with pytest.raises(ValueError):
        find_defects(np.zeros((1, 4, 4)), -1.0)


# ---- C entry points -----------------------------------------------------------------------------------------------------
def test_defect_entry_points_validate_on_the_host():
    from taichi_image_amd import _native
    L = _native.lib()
    assert L.mi_isp_version() >= 1400
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = (ctypes.c_void_p * 1)(p)
    ok = _native.Defects(p.value, 1, p.value)
    bad = [_native.Defects(None, 3, p.value), _native.Defects(p.value, 3, None), _native.Defects(p.value, -1, p.value)]
    for d in bad:
        assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, None, None, d, p, 1, None) != 0
        assert b"defect" in L.mi_isp_last_error()
        assert L.mi_isp_defects_fix_cfa(p, 4, 8, 2, d, None) != 0
        assert b"defect" in L.mi_isp_last_error()
        maps = (ctypes.c_void_p * 1)(ctypes.addressof(d))
        counts = (ctypes.c_int32 * 1)(1)
        assert L.mi_isp_defects_fix_packed_batch(one, one, None, 1, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, 8, None, None,
                                                 maps, one, counts, None) != 0
        assert b"defect" in L.mi_isp_last_error()
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, None, None, None, p, 1, None) != 0
    assert L.mi_isp_defects_fix_cfa(p, 4, 8, 2, None, None) != 0
    # output counts and shapes
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, None, None, ok, p, 33, None) != 0
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, None, None, ok, p, -1, None) != 0
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, None, None, ok, None, 2, None) != 0
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 2, 4, 0.0, None, 8, None, None, ok, p, 1, None) != 0
    assert L.mi_isp_defects_fix_packed(p, p, 3, 8, 12, 0, 0, None, 2, 3, 8, 0.0, None, 8, None, None, ok, p, 1, None) != 0
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, p, 0, None, None, ok, p, 1, None) != 0
    assert L.mi_isp_defects_fix_packed(None, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, None, None, ok, p, 1, None) != 0
    assert L.mi_isp_defects_fix_cfa(p, 4, 8, 0, ok, None) != 0                      # u8 is no work dtype
    assert L.mi_isp_defects_fix_cfa(p, 0, 8, 2, ok, None) != 0
    assert L.mi_isp_defects_fix_cfa(p, 4, 8, 2, _native.Defects(p.value, 33, p.value), None) != 0
    lv = _native.levels_arg([0, 0, 0, 4095], 4095)
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, lv, None, ok, p, 1, None) != 0
    assert b"level" in L.mi_isp_last_error()
    assert L.mi_isp_defects_fix_packed_batch(None, None, None, -1, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, 8, None, None, None,
                                             None, None, None) != 0
    # nothing to do: no frames, or a frame whose map lists no outputs (no launch, no device needed)
    assert L.mi_isp_defects_fix_packed_batch(None, None, None, 0, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, 8, None, None, None,
                                             None, None, None) == 0
    assert L.mi_isp_defects_fix_packed(p, p, 4, 8, 12, 0, 0, None, 2, 4, 8, 0.0, None, 8, None, None, ok, p, 0, None) == 0
    assert L.mi_isp_defects_fix_cfa(p, 4, 8, 2, _native.Defects(None, 0, None), None) == 0


# ---- the scan CLI -------------------------------------------------------------------------------------------------------
def test_scan_defect_pixels_validated_before_any_frame(tmp_path, monkeypatch):
    from taichi_image_amd.scripts import tonemap_scan as ts
    for cam in ("cam0", "cam1"):
        (tmp_path / "scan" / cam).mkdir(parents=True)
        (tmp_path / "scan" / cam / "f0.raw").write_bytes(b"\0" * 12)

    def no_frames(*a, **k):
        raise AssertionError("a frame was read before the defect files were checked")

    monkeypatch.setattr(ts.ScanIndex, "groups", no_frames)
    dp = tmp_path / "dp"
    dp.mkdir()
    base = ["--scan", str(tmp_path / "scan"), "--width", "8", "--defect-pixels", str(dp), "--device", "cpu"]
    for name, arr in (("cam0.npy", np.array([[0, 8]])), ("cam0.npy", np.array([[0, 1, 2]])),
                      ("cam0.npy", np.array([[0.5, 1.0]])), ("cam0.npy", np.array([[-1, 0]])),
                      ("other.npy", np.array([[0, 0]]))):
        for f in dp.iterdir():
            f.unlink()
        np.save(dp / name, arr)
        with pytest.raises(ValueError):
            ts.main(base)
    for f in dp.iterdir():
        f.unlink()
    with pytest.raises(FileNotFoundError):
        ts.main(["--scan", str(tmp_path / "scan"), "--defect-pixels", str(tmp_path / "missing"), "--device", "cpu"])
    np.save(dp / "cam1.npy", np.array([[0, 2], [1, 7]]))
    maps = ts.load_defect_pixels(dp, ts.ScanIndex.of_scan(tmp_path / "scan").cameras, 8)
    assert list(maps) == ["cam1"] and maps["cam1"].tolist() == [[0, 2], [1, 7]]
