"""Local tone mapping without a GPU: the settings' checks, properties of the NumPy restatement of the contract
(tests/local_tonemap_ref.py), the halo test on a step edge and the mutation record.

`python -m tests.test_local_tonemap_cpu` prints profiles/local_tonemap_mutations.txt."""
import numpy as np
import pytest

from tests import local_tonemap_ref as R

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ---- settings ------------------------------------------------------------------------------------------------------------
def test_defaults_and_values_as_f32():
    from taichi_image_amd import LocalTonemap
    s = LocalTonemap()
    assert (s.strength, s.white, s.floor, s.anchor, s.cell, s.bins) == (0.5, 1.0, 2.0 ** -10, 1.0, 32, 16)
    s = LocalTonemap(0.3, white=2, floor=0.001, anchor=0.18, cell=8, bins=32)
    assert s.strength == float(f32(0.3)) and s.floor == float(f32(0.001)) and s.anchor == float(f32(0.18))
    assert s.white == 2.0 and s.grid_shape(130, 66) == (17, 9, 32)
    a = s._arg()
    assert (a.strength, a.white, a.floor, a.anchor, a.cell, a.bins) == (s.strength, 2.0, s.floor, s.anchor, 8, 32)
    r = R.as_settings(s)
    assert (r.span, r.cell, r.bins) == (int(R.Settings(white=2, floor=0.001).li(f32(2))), 8, 32)


@pytest.mark.parametrize("kw", [
    dict(strength=True), dict(strength="0.5"), dict(strength=None), dict(strength=-0.1), dict(strength=1.0001),
    dict(strength=float("nan")), dict(white=0.0), dict(white=-1.0), dict(white=float("inf")), dict(white=1e39),
    dict(white=False), dict(floor=0.0), dict(floor=1e-40), dict(floor=1.0), dict(floor=2.0), dict(floor=float("nan")),
    dict(floor=True), dict(white=1e30, floor=1e-3), dict(white=1.0, floor=2.0 ** -24 * 0.99),
    dict(floor=1.0 - 2.0 ** -24), dict(anchor=2.0), dict(anchor=2.0 ** -11), dict(anchor=float("nan")), dict(anchor=True),
    dict(anchor="1"), dict(cell=12), dict(cell=4), dict(cell=128), dict(cell=32.0), dict(cell=True), dict(bins=1),
    dict(bins=33), dict(bins=16.0), dict(bins=True), dict(bins=None)])
def test_bad_settings_raise_value_error(kw):
    from taichi_image_amd import LocalTonemap
    with pytest.raises(ValueError, match="LocalTonemap"):
        LocalTonemap(**kw)


@pytest.mark.parametrize("kw", [
    dict(strength=0), dict(strength=1), dict(strength=np.float32(0.25)), dict(white=1.0, floor=2.0 ** -24),
    dict(anchor=2.0 ** -10), dict(anchor=1.0), dict(cell=np.int64(64)), dict(bins=2), dict(bins=32),
    dict(white=65504.0, floor=1.0)])
def test_edge_settings_pass(kw):
    from taichi_image_amd import LocalTonemap
    LocalTonemap(**kw)


def test_camera_argument_checks():
    from taichi_image_amd import local_tonemap as M
    assert M.check_local_tonemap(None) is None
    s = M.LocalTonemap()
    assert M.check_local_tonemap(s) is s
    for bad in (True, 0.5, "on", dict(strength=0.5)):
        with pytest.raises(ValueError, match="local_tonemap"):
            M.check_local_tonemap(bad)
    for fn in (M.local_tonemap, M.grids):
        with pytest.raises(ValueError, match="LocalTonemap"):
            fn(np.zeros((4, 4, 3), f32), dict(strength=0.5))
        with pytest.raises(ValueError, match="f16 or f32"):
            fn(np.zeros((4, 4, 3), np.uint8), s)
        with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
            fn(np.zeros((4, 4), f32), s)


# ---- properties of the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_strength_zero_is_the_identity(rng, dtype):
    for content in R.CONTENTS:
        img = R.make_image(rng, 66, 70, content, dtype)
        out = R.local_tonemap(img, dict(strength=0.0, cell=16))
        assert out.dtype == img.dtype and np.array_equal(bits(out), bits(img)), content


def test_gain_bounds_and_one_gain_per_pixel(rng):
    img = R.make_image(rng, 66, 70, "wide", f32)
    for kw in (dict(strength=0.5), dict(strength=1.0, floor=2.0 ** -8, cell=8), dict(strength=0.25, bins=2, cell=64)):
        s = R.as_settings(kw)
        g = R.gain(img, kw)
        top = (float(s.white) / float(s.floor)) ** float(s.strength)
        assert g.min() >= 1.0 and g.max() <= top * (1 + 1e-6), (kw, g.min(), g.max(), top)
        out = R.local_tonemap(img, kw)
        assert np.array_equal(bits(out), bits((img * g[..., None]).astype(f32)))
    g = R.gain(img, dict(strength=0.5, anchor=0.05))               # an anchor inside the range: gains on both sides of 1
    assert g.min() < 1.0 < g.max()


def test_grid_totals(rng):
    for H, W, kw in R.SHAPE_SETTINGS:
        img = R.make_image(rng, H, W, "wide", f32)
        cnt, sm, nb, sb = R.grids(img, kw)
        l, _ = R.log_luma(img, kw)
        assert cnt.shape == R.grid_shape(H, W, kw) and cnt.dtype == np.uint32 and nb.dtype == f32
        assert int(cnt.sum(dtype=np.int64)) == H * W and int(sm.sum(dtype=np.int64)) == int(l.sum())
        assert np.all(nb > 0) or kw["bins"] > 3                    # (a node more than a bin away from every pixel is empty)
        c = kw["cell"]                                             # per cell: as many counts as pixels
        want = np.add.reduceat(np.add.reduceat(np.ones((H, W), np.int64), np.arange(0, H, c), 0), np.arange(0, W, c), 1)
        assert np.array_equal(cnt.sum(axis=2, dtype=np.int64), want)


def test_every_pixel_finds_a_populated_neighbourhood(rng):
    """N > 0 at every pixel of the image (the contract's remark): its own cell and bin are among the taps."""
    for H, W, kw in R.SHAPE_SETTINGS:
        for content in R.CONTENTS:
            img = R.make_image(rng, H, W, content, f32)
            flat = R.gain(img, dict(kw, strength=1.0))
            assert np.all(np.isfinite(flat)) and np.all(flat > 0)


# ---- halo ------------------------------------------------------------------------------------------------------------------
def _edge_gains(seed, bins):
    rng = np.random.default_rng(seed)
    H, W = 128, 256
    img = R.make_image(rng, H, W, "edge", f32)
    g = R.gain(img, dict(strength=0.5, cell=16, bins=bins)).astype(np.float64)
    m = W // 2
    far = (g[:, :32].mean(), g[:, -32:].mean())
    near = (g[:, m - 4:m].mean(axis=0), g[:, m:m + 4].mean(axis=0))
    return far, near


def test_no_halo_at_a_step_edge():
    """A 0.01 / 0.8 step with 2 % noise, strength 0.5, cell 16.  With 16 bins the mean gain of each of the four columns next
    to the edge stays within 0.1 % of the far-field gain of its side (measured over seeds 0 .. 4: at most 0.037 % on the
    dark and 0.028 % on the bright side, which is the scatter of the noise's column means; the margin is 2.7 times that
    and 500 times smaller than the halo below).  With 2 bins, hardly edge-aware, the same columns
    leave it by a factor of more than 2 on the dark side (measured: 10.88 falls to 5.18 .. 4.04) and 1.6 on the bright one
    (1.20 rises to 2.50 .. 2.00): the halo."""
    for seed in range(5):
        far, near = _edge_gains(seed, 16)
        for side in (0, 1):
            rel = np.abs(near[side] / far[side] - 1).max()
            print(f"seed {seed} bins 16 side {side}: far {far[side]:.4f} near {near[side]} rel {rel:.6f}")
            assert rel <= 1e-3, (seed, side, rel)
        assert 10.5 < far[0] < 11.3 and 1.15 < far[1] < 1.25
        far2, near2 = _edge_gains(seed, 2)
        print(f"seed {seed} bins 2: far {far2} near {near2}")
        assert np.all(far2[0] / near2[0] > 2.0) and np.all(near2[1] / far2[1] > 1.6), (seed, near2)


def test_the_pair_is_piecewise_linear_not_a_power_law():
    """A uniform 0.05 image at strength 0.5: the piecewise-linear pair gives 4.80 where the power law gives 4.47."""
    g = R.gain(np.full((64, 64, 3), 0.05, f32), dict(strength=0.5))
    assert np.all(g == g[0, 0]) and abs(float(g[0, 0]) - 4.80) < 0.005
    assert abs((1 / 0.05) ** 0.5 - 4.472) < 0.001


# ---- mutation record -------------------------------------------------------------------------------------------------------
def mutation_table():
    """{mutant: [(input name, grid entries that differ, share of output pixels that differ)]} over the GPU tests' inputs."""
    table = {m: [] for m in R.MUTANTS}
    for name, img, kw in R.gpu_test_inputs():
        g0, o0 = R.grids(img, kw), R.local_tonemap(img, kw)
        for m in R.MUTANTS:
            g, o = R.grids(img, kw, m), R.local_tonemap(img, kw, m)
            entries = sum(int((bits(a) != bits(b)).sum()) for a, b in zip(g0, g))
            table[m].append((name, entries, float((bits(o) != bits(o0)).any(axis=2).mean())))
    return table


def seen(row):
    return row[1] >= 1 or row[2] >= 0.01


def test_every_mutant_is_seen_on_a_gpu_test_input():
    for m, rows in mutation_table().items():
        assert any(seen(r) for r in rows), f"no GPU-test input tells the mutant {m} from the contract"


WHAT = {
    "splat_trunc": "int(z) instead of int(z + 0.5) in the splat",
    "blur_replicate": "replicated instead of zero borders in the blur",
    "lerp_order": "the lerps along y, x, z instead of x, y, z",
    "shift_11": "a shift by 11 instead of 12 in li()",
    "ei_round": "rounding instead of truncation of ei",
    "no_clamp": "the clamp of Y dropped (bins kept inside the grid)",
    "y0_unclamped": "y0 without its max(GH - 2, 0) (a read outside the grid modelled as NaN)",
}

if __name__ == "__main__":
    rows_of = mutation_table()
    n = len(next(iter(rows_of.values())))
    print("Local tone mapping: mutants of the contract, measured on tests/local_tonemap_ref.py (the NumPy restatement) over")
    print(f"the {n} inputs of tests/test_gpu_local_tonemap.py (local_tonemap_ref.gpu_test_inputs()).  A mutant is seen on an")
    print("input when at least one entry of the four grid planes or at least 1 % of the output pixels differ from the")
    print("contract's.  The mutated kernels were not built and run.\n")
    for m, rows in rows_of.items():
        hit = [r for r in rows if seen(r)]
        best = max(rows, key=lambda r: (r[2], r[1]))
        print(f"{m}: {WHAT[m]}")
        print(f"  seen on {len(hit)} of {n} inputs; most on {best[0]}: {best[1]} grid entries, {100 * best[2]:.1f} % of the pixels")
        print("  inputs: " + ", ".join(f"{r[0]} ({r[1]} / {100 * r[2]:.1f} %)" for r in hit[:6]) + (" ..." if len(hit) > 6 else ""))
