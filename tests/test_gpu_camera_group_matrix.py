"""The camera-group kernel (csrc/isp_mega_cam.h, `ISP.process_packed12`) instance by instance: every one of its 12
instances (4 CFA patterns x 3 levels modes) at every row-band remainder and column class, on both sides of every runtime
branch; group sizes around the subsample launch boundary and at the kernel's limit; the subsample kernel on its own; the
sharded route without levels.

The kernel repeats the whole-frame kernel's frame loop (its header says why), and that loop's own tests
(test_gpu_whole_frame_pairs.py, test_gpu_whole_frame_ahead.py) never reach this copy.  With ROWS = 12 rows per wave, five
of them in LDS, and BAND = 512 columns per wave:

  H mod 12   0 a full last band; 2, 4 the last band ends inside the LDS rows; 6 just behind them; 8, 10 in the register rows
  W          8 one active lane; 16; 64 a partial band; 512 one exact band; 520 a band and one lane; 1032 two and one lane

Two references for every case:
  (a) `load_packed12_batch` + `tonemap_reinhard` on a second ISP, bit for bit - u8, p, the metering state: the contract
      isp_mega_cam.h states for itself;
  (b) the oracle chain (load -> c_oracle.IspState.update_metering -> c_oracle.reinhard_isp) at the parity contract of
      tests/util.assert_close (its defaults on u8 and p, rel=2e-5 on the metering state, as
      test_isp_process_packed12_against_the_oracle).  Not on the three shapes whose stride-8 subsample has at most
      4 x 4 samples - (12, 8), (14, 16), (16, 64): a metering state of a handful of samples is near-degenerate, and the
      parity contract says nothing about it.  They keep (a).

Every GPU case asserts that the shape fits the resident grid, that the entry point meant was the one called, and that
the camera group's fault word is 0 after the synchronise.  All the suggested shapes fit an MI355X.

The first tests need no GPU: the shape list has the classes above, every instance meets both sides of every branch, and
- on the oracle alone - the frames give a finite metering state with hi > lo and no NaN in p, and neighbouring cameras of
the group-size cases differ in max_out by 4x or more, so that a camera that took its neighbour's barrier record fails."""
import functools

import numpy as np
import pytest

from oracle import c_oracle, isp_oracle as O
from tests.test_gpu_shading import PER_SITE, ref_load
from tests.util import _count_calls, assert_close, assert_exact, natural_packed12

pytestmark = pytest.mark.skipif(not c_oracle.available(), reason="oracle/liborc_isp.so not built")

ROWS, NL, BAND = 12, 5, 512                             # isp_mega.h: rows per wave, of them in LDS; columns per wave
PATTERNS = {"RGGB": O.RGGB, "GRBG": O.GRBG, "GBRG": O.GBRG, "BGGR": O.BGGR}
# the kernel's LV template argument: 0 no levels, 1 a uniform black level, 2 per site (test_gpu_levels_matrix.GROUP_LEVELS)
LEVELS = {"none": (None, None), "uniform": (300, None), "per_site": (PER_SITE, 3900)}
INSTANCES = [(p, lv) for p in PATTERNS for lv in LEVELS]
SHAPES = [(12, 8), (14, 16), (16, 64), (18, 520), (20, 512), (22, 1032), (26, 520), (34, 1032)]
CCM = O.isp_color_matrix(True, O.DEFAULT_WB, O.DEFAULT_CC)      # what Camera16(correct_colors=True) applies
ALPHA = 0.3
GROUPS = 2


def branches(i):
    """The runtime branches shape i of SHAPES runs, from the bits of its index: gamma by i % 3 (1.0 skips pow_n, 0.5 is an
    even 1 / gamma, 0.6 a fractional one), color_adapt != 0 by bit 0 (with the intensity and light_adapt that go with it),
    the colour matrix by bit 1, keep_images of the first group by bit 2 (the second group takes the other side)."""
    kw = dict(gamma=(1.0, 0.5, 0.6)[i % 3])
    if i & 1:
        kw.update(color_adapt=0.3, intensity=1.2, light_adapt=0.7)
    return kw, bool(i & 2), bool(i & 4)


def oracle_compared(shape):
    """Reference (b) needs a stride-8 subsample of more than 4 x 4 = 16 samples."""
    return -(-shape[0] // 8) * -(-shape[1] // 8) > 16


def case_id(v):
    if isinstance(v, tuple):
        i = SHAPES.index(v)
        kw, cc, keep = branches(i)
        return (f"{v[0]}x{v[1]}-g{kw['gamma']}-ca{kw.get('color_adapt', 0.0)}-{'ccm' if cc else 'noccm'}-"
                f"{'keep' if keep else 'drop'}")
    return str(v)


def _frozen(a):
    a.setflags(write=False)
    return a


def scene_codes(rng, shape, pattern, offset):
    """The 12-bit CFA codes of a bright smooth-plus-noise scene that darkens smoothly to a fifth toward its top left pixel.
    The metering reads image[::8, ::8] only: pixel (0, 0) is then its darkest sample and darker than every pixel off the
    grid as well, so no pixel has a negative gray (whose p is NaN); and none is black (NaN too when light_adapt is 1)."""
    H, W = shape
    codes = O.decode12(natural_packed12(rng, H, W, PATTERNS[pattern], dark=-offset), "u16").astype(np.float64)
    d = np.hypot(np.arange(H)[:, None], np.arange(W)[None, :])
    return np.rint(codes * (0.2 + 0.8 * np.minimum(d / 16.0, 1.0))).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def packed_frame(shape, pattern, group, k):
    """Camera k's frame of a group, every camera at its own offset."""
    rng = np.random.default_rng(7000 + 1000 * group + 10 * k + PATTERNS[pattern])
    return _frozen(O.encode12(scene_codes(rng, shape, pattern, 0.30 + 0.04 * k)))


@functools.lru_cache(maxsize=256)
def ref_image(shape, pattern, levels, cc, group, k):
    """The oracle's load_packed12 of that frame: (H, W, 3) f16."""
    black, white = LEVELS[levels]
    return _frozen(ref_load(packed_frame(shape, pattern, group, k), 12, "f16", PATTERNS[pattern], None, black, white,
                            ccm=CCM if cc else None))


def oracle_chain(refs_per_group, kw, cameras=None):
    """The oracle's rolling metering over the groups and its Reinhard of the cameras asked for:
    per group (metering state, {k: (u8, p)})."""
    st, out = c_oracle.IspState(ALPHA), []
    for refs in refs_per_group:
        m = st.update_metering(list(refs)).copy()
        out.append((m, {k: c_oracle.reinhard_isp(refs[k], m, **kw) for k in (cameras or range(len(refs)))}))
    return out


def assert_usable_metering(m, what):
    assert np.all(np.isfinite(m)), f"{what}: metering state {m}"
    assert m[1] > m[0], f"{what}: bounds {m[0]} .. {m[1]}"


# ---------------------------------------------------------------------------------------------------------------------
# preconditions (no GPU)

def test_shapes_and_branches_cover_every_class():
    """What the GPU cases take for granted about SHAPES and branches(): every instance runs every shape, so these are
    properties of the list alone."""
    assert len(INSTANCES) == 12 and len(set(INSTANCES)) == 12
    assert len(SHAPES) <= 8 and all(H <= 34 and W <= 1032 and H % 2 == 0 and W % 8 == 0 for H, W in SHAPES)
    rem = [H % ROWS for H, _ in SHAPES]
    assert set(rem) == {0, 2, 4, 6, 8, 10}
    assert sum(1 for r in set(rem) if 0 < r <= NL) == 2, "two remainders end the last band inside the LDS rows"
    assert NL + 1 in rem, "one ends it just behind them"
    widths = {W for _, W in SHAPES}
    assert 8 in widths and 16 in widths, "one active lane; two"
    assert any(16 < W < BAND for W in widths), "a partial band"
    assert BAND in widths and BAND + 8 in widths and 2 * BAND + 8 in widths
    assert any(H > ROWS for H, _ in SHAPES) and any(W > BAND for _, W in SHAPES), "more than one wave each way"
    for part in (SHAPES, [s for s in SHAPES if oracle_compared(s)]):         # (both references see both sides)
        seen = [branches(SHAPES.index(s)) for s in part]
        assert {kw["gamma"] for kw, _, _ in seen} == {1.0, 0.5, 0.6}
        assert {kw.get("color_adapt", 0.0) for kw, _, _ in seen} == {0.0, 0.3}
        assert {cc for _, cc, _ in seen} == {False, True}
        assert {keep for _, _, keep in seen} == {False, True}
    bare = [s for s in SHAPES if not oracle_compared(s)]
    assert len(bare) <= 3 and all(-(-H // 8) * -(-W // 8) <= 16 for H, W in bare)


@pytest.mark.parametrize("pattern,levels", INSTANCES)
def test_frames_give_the_oracle_a_usable_metering_state(pattern, levels):
    """For every shape that gets reference (b): over the groups of the rolling metering the oracle's state is finite with
    hi > lo, and no p is NaN (NaNs would have to coincide; a frame without them compares every pixel)."""
    for i, shape in enumerate(SHAPES):
        if not oracle_compared(shape):
            continue
        kw, cc, _ = branches(i)
        refs = [[ref_image(shape, pattern, levels, cc, g, k) for k in range(2)] for g in range(GROUPS)]
        for g, (m, cams) in enumerate(oracle_chain(refs, kw)):
            assert_usable_metering(m, f"{shape} {pattern} {levels} group {g}")
            for k, (u8, p) in cams.items():
                assert not np.isnan(p).any(), f"{shape} {pattern} {levels} group {g} camera {k}: NaN in p"


# ---------------------------------------------------------------------------------------------------------------------
# 1. instance x geometry

@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def _dev(dev, packed):
    import torch
    return torch.from_numpy(np.array(packed)).to(dev)                  # (a copy: the cached frames are read-only)


def _levels_arg(ti, levels):
    from taichi_image_amd import _native
    return _native.levels_arg(*ti.camera_isp._check_levels(*LEVELS[levels], 12)) if levels != "none" else None


def _assert_fits(ti, shape, pattern, levels):
    from taichi_image_amd import _native
    L = _native.lib()
    lv = _levels_arg(ti, levels)
    if lv is None:
        assert L.mi_isp_camera_group_fits(shape[0], shape[1], PATTERNS[pattern], ti.types.f16.code, 8) == 1
    else:
        assert L.mi_isp_camera_group_fits_levels(shape[0], shape[1], PATTERNS[pattern], ti.types.f16.code, 8, lv) == 1


def _camera(ti, dev, pattern, levels, cc=False, **kw):
    black, white = LEVELS[levels]
    isp = ti.Camera16(ti.BayerPattern(PATTERNS[pattern]), moving_alpha=ALPHA, correct_colors=cc, device=dev,
                      black_level=black, white_level=white, **kw)
    if cc:
        assert np.array_equal(np.asarray(isp.color_correct_matrix, np.float64).reshape(-1), CCM.reshape(-1))
    return isp


def _entry(name, levels):
    return name if levels == "none" else name + "_levels"


def run_groups(ti, dev, monkeypatch, packs_per_group, pattern, levels, cc, kw, keep_first, what):
    """The groups through process_packed12 on one ISP and through the two calls on another: bit for bit (reference (a)).
    Returns per group (metering state, u8 outputs, images or None) of the camera-group kernel, on the host."""
    import torch
    from taichi_image_amd import _native
    L = _native.lib()
    a, b = _camera(ti, dev, pattern, levels, cc), _camera(ti, dev, pattern, levels, cc)
    fused = _count_calls(monkeypatch, _entry("mi_isp_camera_group_reinhard", levels))
    got = []
    for g, packs in enumerate(packs_per_group):
        frames = [_dev(dev, p) for p in packs]
        keep = keep_first == (g % 2 == 0)
        res = a.process_packed12(frames, keep_images=keep, **kw)
        assert len(fused) == g + 1, f"{what}: process_packed12 did not take the camera-group kernel"
        outs, images = res if keep else (res, None)
        want_images = b.load_packed12_batch(frames)
        want = b.tonemap_reinhard(want_images, **kw)
        torch.cuda.synchronize()
        assert L.mi_isp_camera_group_faults(0) == 0
        assert torch.equal(a.metrics.view(torch.int32), b.metrics.view(torch.int32)), f"{what} group {g}: metering state"
        assert len(outs) == len(frames)
        for k in range(len(frames)):
            assert torch.equal(outs[k], want[k]), f"{what} group {g} camera {k}: u8 output"
            if keep:
                assert torch.equal(images[k].view(torch.int16), want_images[k].view(torch.int16)), \
                    f"{what} group {g} camera {k}: p"
        got.append((a.metrics.cpu().numpy(), [o.cpu().numpy() for o in outs],
                    [im.cpu().numpy() for im in images] if keep else None))
    return got


def compare_with_oracle(got, chain, what):
    """Reference (b): the project's parity numbers."""
    for g, ((m, outs, images), (ref_m, cams)) in enumerate(zip(got, chain)):
        assert_close(m, ref_m, f"{what} group {g}: metrics vs oracle", rel=2e-5)
        for k, (ref_u8, ref_p) in cams.items():
            assert_close(outs[k], ref_u8, f"{what} group {g} camera {k}: u8 vs oracle")
            if images is not None:
                assert_close(images[k], ref_p, f"{what} group {g} camera {k}: p vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
@pytest.mark.parametrize("pattern,levels", INSTANCES)
def test_instance_at_every_geometry(ti, dev, monkeypatch, pattern, levels, shape):
    """One instance at one shape, the runtime branches by the shape's index: two groups of two cameras of a rolling
    metering, against the two calls bit for bit and against the oracle chain."""
    kw, cc, keep_first = branches(SHAPES.index(shape))
    what = f"{pattern} {levels} {shape}"
    _assert_fits(ti, shape, pattern, levels)
    packs = [[packed_frame(shape, pattern, g, k) for k in range(2)] for g in range(GROUPS)]
    got = run_groups(ti, dev, monkeypatch, packs, pattern, levels, cc, kw, keep_first, what)
    assert (got[0][2] is not None) == keep_first and (got[1][2] is not None) != keep_first
    if oracle_compared(shape):
        refs = [[ref_image(shape, pattern, levels, cc, g, k) for k in range(2)] for g in range(GROUPS)]
        compare_with_oracle(got, oracle_chain(refs, kw), what)


# ---------------------------------------------------------------------------------------------------------------------
# 2. group size and per-camera max_out

# Reinhard compresses: with its default arguments a camera at a tenth of the range still reaches half of its neighbour's
# max_out.  light_adapt = 0 (one adaptation level for the whole group) and intensity = -1 keep p close to linear in the pixel.
GROUP_SHAPE, GROUP_PATTERN, GROUP_KW = (26, 520), "GRBG", dict(gamma=0.6, intensity=-1.0, light_adapt=0.0)
GROUP_SIZES = [1, 7, 8, 9, 63, 64]                      # LOAD_BATCH = 8 cameras per subsample launch, MAX_BATCH = 64 per call
DIM_GAIN = 0.1                                          # odd cameras: a tenth of the code range


@functools.lru_cache(maxsize=None)
def gain_frame(group, k):
    """Camera k of a group-size case: even k at full range, odd k with its CFA codes scaled to a tenth
    (test_gpu_whole_frame_ahead.frame: scale the CFA, then encode)."""
    rng = np.random.default_rng(9000 + 1000 * group + k)
    cfa = scene_codes(rng, GROUP_SHAPE, GROUP_PATTERN, 0.30 + 0.002 * k).astype(np.float64) * (DIM_GAIN if k % 2 else 1.0)
    return _frozen(O.encode12(np.rint(cfa).astype(np.uint16)))


@functools.lru_cache(maxsize=None)
def gain_ref(group, k):
    return _frozen(O.isp_load_packed12(gain_frame(group, k), "f16", PATTERNS[GROUP_PATTERN]))


def oracle_cameras(n):
    return sorted({0, 7, 8, n - 1}) if n >= 63 else list(range(n))


@pytest.mark.parametrize("n", GROUP_SIZES)
def test_neighbouring_cameras_differ_in_max_out(n):
    """On the oracle: max_out (the largest p of a camera: camera_isp.py:213; here from p as stored, f16 - within 2^-11 of
    it) of neighbouring cameras differs by 4x or more, in both groups."""
    refs = [[gain_ref(g, k) for k in range(n)] for g in range(GROUPS)]
    for g, (m, cams) in enumerate(oracle_chain(refs, GROUP_KW)):
        assert_usable_metering(m, f"n {n} group {g}")
        mx = []
        for k in range(n):
            p = cams[k][1].astype(np.float32)
            assert not np.isnan(p).any(), f"n {n} group {g} camera {k}: NaN in p"
            mx.append(float(p.max()))
        for k in range(1, n):
            big, small = max(mx[k - 1], mx[k]), min(mx[k - 1], mx[k])
            assert small > 0 and big >= 4.0 * small, f"n {n} group {g}: max_out of cameras {k - 1}, {k}: {mx[k - 1]}, {mx[k]}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", GROUP_SIZES)
def test_group_sizes_and_per_camera_max_out(ti, dev, monkeypatch, n):
    """n cameras in one launch, bright and dim alternating: every camera against the two calls bit for bit, and against
    the oracle (for 63 and 64 cameras: the first, those on both sides of the subsample launch boundary, the last)."""
    what = f"n {n}"
    _assert_fits(ti, GROUP_SHAPE, GROUP_PATTERN, "none")
    packs = [[gain_frame(g, k) for k in range(n)] for g in range(GROUPS)]
    got = run_groups(ti, dev, monkeypatch, packs, GROUP_PATTERN, "none", False, GROUP_KW, True, what)
    refs = [[gain_ref(g, k) for k in range(n)] for g in range(GROUPS)]
    compare_with_oracle(got, oracle_chain(refs, GROUP_KW, oracle_cameras(n)), what)


@pytest.mark.gpu
def test_more_cameras_than_one_launch_takes_the_two_calls(ti, dev, monkeypatch):
    """65 cameras: process_packed12 gives the two calls' results bit for bit without calling the camera-group kernel;
    no frame at all keeps its assertion."""
    import torch
    from taichi_image_amd import _native
    n = 65
    a, b = _camera(ti, dev, GROUP_PATTERN, "none"), _camera(ti, dev, GROUP_PATTERN, "none")
    fused = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard")
    frames = [_dev(dev, gain_frame(0, k)) for k in range(n)]
    outs, images = a.process_packed12(frames, keep_images=True, **GROUP_KW)
    want_images = b.load_packed12_batch(frames)
    want = b.tonemap_reinhard(want_images, **GROUP_KW)
    torch.cuda.synchronize()
    assert fused == [], "65 cameras went to the camera-group kernel"
    assert _native.lib().mi_isp_camera_group_faults(0) == 0
    assert torch.equal(a.metrics.view(torch.int32), b.metrics.view(torch.int32))
    assert len(outs) == n and len(images) == n
    for k in range(n):
        assert torch.equal(outs[k], want[k]), f"camera {k}: u8 output"
        assert torch.equal(images[k].view(torch.int16), want_images[k].view(torch.int16)), f"camera {k}: p"
    with pytest.raises(AssertionError):
        a.process_packed12([], **GROUP_KW)
    assert fused == []


@pytest.mark.gpu
def test_entry_point_refuses_65_cameras_before_anything_is_launched(ti, dev):
    """mi_isp_camera_group_reinhard with n = 65: non-zero, a message, and neither the state nor an output written."""
    import torch
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = GROUP_SHAPE
    n = 65
    _assert_fits(ti, GROUP_SHAPE, GROUP_PATTERN, "none")
    src = _dev(dev, gain_frame(0, 0))
    outs = [torch.full((H, W, 3), 0x5A, dtype=torch.uint8, device=dev) for _ in range(n)]
    images = [torch.full((H, W, 3), 3.0, dtype=torch.float16, device=dev) for _ in range(n)]
    prev = torch.zeros(9, dtype=torch.float32, device=dev)
    state = torch.full((9,), -7.0, dtype=torch.float32, device=dev)
    scratch = torch.zeros(int(L.mi_isp_camera_group_scratch_bytes(n, H, W)), dtype=torch.uint8, device=dev)
    ws = _native.workspace(H, W, dev, slots=n + 1)
    rc = L.mi_isp_camera_group_reinhard(_native.ptr_array([src] * n), _native.ptr_array(images), _native.ptr_array(outs), n, H, W,
                                        PATTERNS[GROUP_PATTERN], None, prev.data_ptr(), state.data_ptr(), 0.0, 0.6, 1.0, 1.0,
                                        0.0, scratch.data_ptr(), ws.data_ptr(), _native.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.mi_isp_last_error().decode("utf-8", "replace")
    assert "camera_group_reinhard" in msg and "cameras per call" in msg, msg
    assert L.mi_isp_camera_group_faults(0) == 0
    assert torch.equal(state, torch.full_like(state, -7.0)), "the metering state was written"
    assert not scratch.any(), "the subsample was launched"
    for k in range(n):
        assert bool((outs[k] == 0x5A).all()) and bool((images[k] == 3.0).all()), f"camera {k}'s buffers were written"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the subsample kernel, directly

@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pattern,levels", INSTANCES)
def test_subsample_kernel_is_the_image_at_stride_8(ti, dev, pattern, levels, shape):
    """mi_isp_camera_group_subsample(_levels) on 9 cameras (two launches: 8 and 1), with and without the colour matrix:
    every camera's block of the scratch is image[::8, ::8] of the loaded image, bit for bit, and the oracle's."""
    import torch
    from taichi_image_amd import _native
    L = _native.lib()
    H, W = shape
    n = 9
    hs, wsub = -(-H // 8), -(-W // 8)
    _assert_fits(ti, shape, pattern, levels)
    lv = _levels_arg(ti, levels)
    per = int(L.mi_isp_camera_group_scratch_bytes(1, H, W))
    assert per >= hs * wsub * 6 and per % 256 == 0 and int(L.mi_isp_camera_group_scratch_bytes(n, H, W)) == n * per
    frames = [_dev(dev, packed_frame(shape, pattern, 0, k)) for k in range(n)]
    for cc in (False, True):
        isp = _camera(ti, dev, pattern, levels, cc)
        scratch = torch.full((n * per,), 0xFF, dtype=torch.uint8, device=dev)      # (f16 NaN where nothing is written)
        args = (_native.ptr_array(frames), n, H, W, PATTERNS[pattern], _native.ccm_arg(isp.color_correct_matrix),
                scratch.data_ptr())
        if lv is None:
            rc = L.mi_isp_camera_group_subsample(*args, _native.stream_ptr(dev))
        else:
            rc = L.mi_isp_camera_group_subsample_levels(*args, lv, _native.stream_ptr(dev))
        _native.check(rc)
        loaded = isp.load_packed12_batch(frames)
        torch.cuda.synchronize()
        assert L.mi_isp_camera_group_faults(0) == 0
        for k in range(n):
            what = f"{pattern} {levels} {shape} ccm {cc} camera {k}"
            block = scratch[k * per:k * per + hs * wsub * 6].view(torch.float16).view(hs, wsub, 3)
            assert torch.equal(block.view(torch.int16), loaded[k][::8, ::8].contiguous().view(torch.int16)), \
                f"{what}: not the loaded image's subsample"
            assert_exact(block.cpu().numpy(), np.ascontiguousarray(ref_image(shape, pattern, levels, cc, 0, k)[::8, ::8]),
                         f"{what}: vs the oracle")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the sharded route without levels

SHARDED_SHAPES = [(14, 16), (18, 520), (22, 1032)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHARDED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_sharded_camera_group_without_levels(ti, dev, monkeypatch, pattern, shape):
    """The sharded camera group on one rank (test_gpu_levels_matrix.test_sharded_camera_group_levels, here without levels:
    the plain entry points): subsample -> the sharded metering -> tonemap gives the metering state and the outputs of the
    unsharded call, over three steps."""
    import torch
    from taichi_image_amd import _native
    assert {s[1] for s in SHARDED_SHAPES} == {16, BAND + 8, 2 * BAND + 8} and set(SHARDED_SHAPES) <= set(SHAPES)
    n = 3
    _assert_fits(ti, shape, pattern, "none")
    a = _camera(ti, dev, pattern, "none")
    b = _camera(ti, dev, pattern, "none", process_group=object())               # one "rank"
    fused = _count_calls(monkeypatch, "mi_isp_camera_group_reinhard")
    sub = _count_calls(monkeypatch, "mi_isp_camera_group_subsample")
    tonemap = _count_calls(monkeypatch, "mi_isp_camera_group_tonemap")
    with_levels = [_count_calls(monkeypatch, "mi_isp_camera_group_" + s + "_levels") for s in ("reinhard", "subsample", "tonemap")]
    for step in range(3):
        frames = [_dev(dev, packed_frame(shape, pattern, step, k)) for k in range(n)]
        oa = a.process_packed12(frames, gamma=0.6)
        assert len(fused) == step + 1 and len(sub) == step and len(tonemap) == step, "the unsharded camera took another path"
        ob = b.process_packed12(frames, gamma=0.6)
        assert len(sub) == step + 1 and len(tonemap) == step + 1 and len(fused) == step + 1, "the sharded camera group was not taken"
        assert_close(b.metrics.cpu().numpy(), a.metrics.cpu().numpy(), f"metering state, step {step}", rel=1e-5)
        for k, (x, y) in enumerate(zip(oa, ob)):
            assert_close(y.cpu().numpy(), x.cpu().numpy(), f"u8 output {k}, step {step}")
    torch.cuda.synchronize()
    assert with_levels == [[], [], []]
    assert _native.lib().mi_isp_camera_group_faults(0) == 0
