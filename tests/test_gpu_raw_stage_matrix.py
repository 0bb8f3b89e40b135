"""The raw-domain stages (csrc/isp_exposure_merge.hip, isp_highlights.hip, isp_chromatic.hip, isp_temporal.hip,
isp_denoise.hip), instance by instance against their NumPy references, and the host tables around them.

1. Every (SRC, OUT) instance a raw entry point can reach, through the C ABI: mi_isp_merge_raw (E = 3),
   mi_isp_highlights_raw ("rebuild"), mi_isp_chromatic_raw and mi_isp_temporal_raw for every source kind (packed 12,
   packed 12 IDS, packed 16, 16U, 16F, 32F) and every output (OUT_F16, OUT_F32, OUT_PLAIN), with levels where the kind
   takes them, a 4-site shading grid on the gained outputs and the seam defect map: the reference's y bit for bit (plain),
   its gained cast bit for bit (F16 / F32).  The _raw entries do not run the defect fix-up, and the references define y at
   listed sites, so every pixel is compared.  Temporal runs two steps (a null history, then the first step's plane) and
   compares the new history in every case.  mi_isp_denoise_raw_batch with n = 1 for every kind x {F16, F32} x radius
   {1, 2} holds the filter's own bound (tests/denoise_ref.py) at the unlisted sites.
   Shapes: 66 x 70 (two tile rows and columns of the 64 x 64 tile with a 2 x 6 remainder), 2 x 4 (one block, mostly
   outside; with the map - which lists all eight sites - and without one), and for the kinds that take odd sizes 67 x 69
   (decode_pair's single-pixel arm, the narrow store).
   Not reached here: SRC_CFA_F16 / SRC_CFA_F32 belong to the *_cfa entries (merge_cfa, reconstruct_cfa, correct_cfa,
   temporal_cfa, denoise_cfa), which the feature tests cover with OUT of the same dtype; <CFA_F16, OUT_F32>,
   <CFA_F32, OUT_F16> and <CFA_*, OUT_PLAIN> are instantiated, but no entry point dispatches to them.  dn::denoise_kernel
   has no plain output.
2. Every position a stage takes in ISP._raw_chain that the feature tests leave out, and the chains H, D and HD of one or
   two stages (every loader with a raw stage on takes that one route), through the loaders of Camera16 and
   Camera32 at 66 x 70 (CHAINS below): the references composed in _raw_chain's order; every intermediate a chain exposes
   (the plain f32 output of each stage that is not the last, read from the tensors the wrapped entry point wrote, and the
   temporal history) bit for bit, the final CFA bit for bit - or, behind raw noise reduction, within its bound - and one
   launch per stage and load.
3. The second launch of the five batched entry points no test takes beyond their per-launch limit (temporal 32, exposure
   merge 16, AWB statistics 32, lens 32 per border mode, defect fix-up 32 mapped frames): every frame of a call with more
   frames than one launch takes equals its own single-frame call.
4. The alignment forks: em::merge_kernel's narrow store on an even width with a destination one element off, and
   ltm's element-wise route on W % 4 == 0 with an image one element off its allocation.

The first tests need no GPU: the tables are the full cross products, the launch limits are the ones the sources state, and
- on the references alone - every generated input exercises its operator.  profiles/raw_stage_matrix_mutations.txt
records the deliberate edits of the library these tests were run against."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import chromatic_ref as CR
from tests import denoise_ref as D
from tests import exposure_merge_ref as M
from tests import highlights_ref as HR
from tests import local_tonemap_ref as LR
from tests import temporal_ref as T
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_denoise import call, capture
from tests.test_gpu_exposure_merge import assert_exercised, bracket, load as load_bracket
from tests.test_gpu_shading import make_grid, pixel_gains
from tests.test_gpu_temporal import cfa_of, check_image, encode, seam_defects
from tests.util import _count_calls, assert_exact

gpu = pytest.mark.gpu
f32 = np.float32

CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
KINDS = ["p12", "ids", "p16", "16u", "16f", "32f"]
PACKED = ("p12", "ids", "p16")
OUTS = ["f16", "f32", "plain"]
STAGES = ["merge", "highlights", "chromatic", "temporal"]
STAGE_CASES = [(s, k, o) for s in STAGES for k in KINDS for o in OUTS]
DENOISE_CASES = [(k, w, r) for k in KINDS for w in ("f16", "f32") for r in (1, 2)]
RATIOS = (1, 4, 16)
GAIN, READ_NOISE = 2.4e-4, 1.5e-3
WB = np.array([1.8, 1.0, 2.1])
CLIP = 0.98
PATTERN = {k: i % 4 for i, k in enumerate(KINDS)}        # every Bayer pattern among the kinds
UNIT = {k: 1000.0 if k == "16f" else 1.0 for k in KINDS}  # load_16f's x is the code, 0 .. 1000
SEAMS = (66, 70)

# the chains of section 2 -> the kind that runs them besides p12
CHAINS = {"MH": "ids", "MC": "16f", "MD": "p16", "CT": "32f", "HT": "16u", "TD": "ids", "MCT": "p16", "HTD": "32f",
          "H": "p16", "D": "16f", "HD": "16u"}
CHAIN_CASES = [(c, k) for c, other in CHAINS.items() for k in ("p12", other)]
ENTRY = {"M": ("mi_isp_merge_raw_batch", 1), "H": ("mi_isp_highlights_raw_batch", 1), "C": ("mi_isp_chromatic_raw_batch", 1),
         "T": ("mi_isp_temporal_raw_batch", 2), "D": ("mi_isp_denoise_raw_batch", 1)}     # entry point, its output list

# frames per launch, as the sources state them (test_launch_limits_are_the_sources)
LIMITS = {"isp_temporal.h": ("MAX_FRAMES", 32), "isp_exposure_merge.h": ("MAX_BRACKETS", 16), "isp_awb.h": ("MAX_FRAMES", 32),
          "isp_lens.h": ("MAX_CAMS", 32), "isp_defects.h": ("MAX_CAMS", 32)}
N_TEMPORAL, N_MERGE, N_AWB, N_LENS, N_DEFECTS, N_MAPPED = 33, 17, 33, 35, 36, 33


def _rng(*key):
    return np.random.default_rng([20261, *[int(k) for k in key]])


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def ti():
    return _ti()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def to_dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)              # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def grid():
    return _frozen(make_grid(_rng(7), 5, 7, 4))


class _EvenFrame:
    """seam_defects' DefectMap for an odd-sized frame (a DefectMap has an even shape): the map of the next even frame with
    every site inside the odd one.  Its mask has the frame's ceil(W / 32) words per row and one spare row."""
    @staticmethod
    def DefectMap(sites, shape):
        H, W = shape
        assert (W + 31) // 32 == (W + W % 2 + 31) // 32
        return _ti().DefectMap(sites, (H + H % 2, W + W % 2))


@functools.lru_cache(maxsize=None)
def the_map(H, W):
    return seam_defects(_EvenFrame, _rng(9, H, W), H, W)


def the_mask(H, W):
    return the_map(H, W).mask()[:H, :W]


def gained(y, work):
    """The gained cast of a stage's y: what the last stage of a route stores."""
    return O.cast_out((y * pixel_gains(grid(), *y.shape)).astype(f32), work)


def encode_any(kind, u):
    """encode(kind, u, levels=True) at any size: an odd-sized frame is cut from the next even one (levels are per site, so
    the cut keeps them)."""
    H, W = u.shape
    if H % 2 == 0 and W % 2 == 0:
        return encode(kind, u, levels=True)
    assert kind not in PACKED
    src, x, black, white = encode(kind, np.pad(u, ((0, H % 2), (0, W % 2)), mode="edge"), levels=True)
    return np.ascontiguousarray(src[:H, :W]), np.ascontiguousarray(x[:H, :W]), black, white


def shape_cases(kind):
    """(H, W, with the map) of a section 1 case."""
    return [(66, 70, True), (2, 4, True), (2, 4, False)] + ([] if kind in PACKED else [(67, 69, True)])


def stage_settings(stage, kind, H, W, radius=1):
    ti, unit = _ti(), UNIT[kind]
    if stage == "merge":
        return ti.ExposureMerge(RATIOS, GAIN * unit, READ_NOISE * unit, saturation=0.9 * unit)
    if stage == "highlights":
        return ti.Highlights("rebuild", CLIP * unit)
    if stage == "chromatic":
        k = CR.frame_settings(H, W)
        return ti.ChromaticAberration(k.red, k.blue)
    if stage == "temporal":
        return ti.TemporalDenoise(GAIN * unit, READ_NOISE * unit)
    if radius == 1:
        return ti.RawDenoise(0.002 * unit, 0.01 * unit, strength=1.5, radius=1)
    return ti.RawDenoise(0.002 * unit, 0.01 * unit, strength=1.0, radius=2, spatial_sigma=1.5)


@functools.lru_cache(maxsize=None)
def stage_case(stage, kind, H, W, mapped):
    """The inputs of a section 1 case and the reference's y: dict(srcs, xs, black, white, ys).  merge: srcs / xs hold the
    bracket and ys its one y; temporal: two frames and the two ys; the others one frame."""
    rng = _rng(1 + (STAGES + ["denoise"]).index(stage), KINDS.index(kind), H, W)
    mask = the_mask(H, W) if mapped else None
    pattern = PATTERN[kind]
    if stage == "merge":
        us = M.make_bracket(rng, H, W, RATIOS, GAIN, READ_NOISE)
    elif stage == "highlights":
        lo = int(0.985 * 4095) + 1
        us = [HR.make_codes(rng, H, W, 4095, lo, pattern).astype(np.float64) / 4095.0]
    elif stage == "chromatic":
        us = [rng.random((H, W))]
    elif stage == "temporal":
        us = T.make_sequence(rng, H, W, 2, GAIN, READ_NOISE)
    else:
        us = [(rng.random((H, W)) * 0.6 + 0.2 + rng.normal(0, 0.02, (H, W))).clip(0, 1)]
    enc = [encode_any(kind, u) for u in us]
    xs = [e[1] for e in enc]
    s = stage_settings(stage, kind, H, W)
    if stage == "merge":
        ys = [M.merge(xs, s, mask)]
    elif stage == "highlights":
        ys = [HR.reconstruct(xs[0], pattern, f32(WB), "rebuild", s.clip, mask)]
    elif stage == "chromatic":
        ys = [CR.correct(xs[0], pattern, s, mask)]
    elif stage == "temporal":
        ys = T.run(xs, s, mask)
    else:
        ys = []
    return dict(srcs=[_frozen(e[0]) for e in enc], xs=[_frozen(x) for x in xs], black=enc[0][2], white=enc[0][3],
                ys=[_frozen(y) for y in ys], mask=mask)


# ---- without a GPU: the tables and the inputs ---------------------------------------------------------------------------
def test_the_matrix_is_the_full_cross_product():
    assert STAGE_CASES == list(itertools.product(STAGES, KINDS, OUTS)) and len(set(STAGE_CASES)) == 4 * 6 * 3
    assert DENOISE_CASES == list(itertools.product(KINDS, ("f16", "f32"), (1, 2))) and len(set(DENOISE_CASES)) == 24
    assert KINDS == ["p12", "ids", "p16", "16u", "16f", "32f"] and OUTS == ["f16", "f32", "plain"]
    for kind in KINDS:
        shapes = {(H, W) for H, W, _ in shape_cases(kind)}
        assert shapes == {(66, 70), (2, 4)} | (set() if kind in PACKED else {(67, 69)})
        assert all(H * W <= 67 * 69 for H, W in shapes)
    assert sorted(PATTERN.values()) == [0, 0, 1, 1, 2, 3]
    # the parametrisation of the GPU tests is these tables
    marks = {m.args[0]: m.args[1] for m in test_stage_instance.pytestmark if m.name == "parametrize"}
    assert marks["stage,kind,out"] is STAGE_CASES
    marks = {m.args[0]: m.args[1] for m in test_denoise_instance.pytestmark if m.name == "parametrize"}
    assert marks["kind,work,radius"] is DENOISE_CASES


def test_the_chains_and_their_kinds():
    assert list(CHAINS) == ["MH", "MC", "MD", "CT", "HT", "TD", "MCT", "HTD", "H", "D", "HD"]
    assert {"ids", "p16", "16f", "32f"} <= set(CHAINS.values()) and "p12" not in CHAINS.values()
    assert CHAIN_CASES == [(c, k) for c in CHAINS for k in ("p12", CHAINS[c])] and len(set(CHAIN_CASES)) == 22
    for chain in CHAINS:                                   # _raw_chain's order, every stage at most once
        assert [s for s in "MHCTD" if s in chain] == list(chain)
    marks = {m.args[0]: m.args[1] for m in test_chain_positions.pytestmark if m.name == "parametrize"}
    assert marks["chain,kind"] is CHAIN_CASES and marks["cam,work"] is CAMS


def test_launch_limits_are_the_sources():
    """The frame counts of section 3 leave the first launch of their entry point."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "taichi_image_amd", "csrc")
    for name, (const, value) in LIMITS.items():
        with open(os.path.join(csrc, name)) as f:
            found = re.findall(rf"constexpr int {const} = (\d+);", f.read())
        assert found == [str(value)], f"{name}: {const} is {found}, the tests assume {value}"
    assert N_TEMPORAL > 32 and N_AWB > 32 and N_MERGE > 16 and N_MAPPED > 32 and N_DEFECTS == N_MAPPED + 3
    for last in ("constant", "replicate"):
        borders = lens_borders(last)
        assert len(borders) == N_LENS and borders.count("constant") == 33 and borders.count("replicate") == 2
        assert borders[-1] == last
        full = [i for i in range(N_LENS) if borders[:i + 1].count("constant") == 32][0]
        assert 0 < borders[:full].count("replicate") < 32, "the replicate bucket is open when the constant one flushes"
        assert "constant" in borders[full + 1:], "a constant frame follows the flush"
    for last_mapped in (False, True):
        maps = defect_slots(last_mapped)
        assert len(maps) == N_DEFECTS and sum(maps) == N_MAPPED and not maps[0] and maps[-1] == last_mapped
        full = [i for i in range(N_DEFECTS) if sum(maps[:i + 1]) == 32][0]
        assert not all(maps[1:full]), "a frame without a map among the first 32 mapped ones"
        assert sum(maps[full + 1:]) == 1, "one mapped frame is left for the second launch"


@pytest.mark.parametrize("kind", KINDS)
def test_merge_inputs_exercise_the_operator(kind):
    for H, W, mapped in shape_cases(kind):
        c = stage_case("merge", kind, H, W, mapped)
        assert H * W < 4096 or c["xs"][0].size >= 4096
        assert_exercised(c["xs"], stage_settings("merge", kind, H, W), c["mask"], f"merge {kind} {H}x{W}")


@pytest.mark.parametrize("kind", KINDS)
def test_highlights_inputs_exercise_the_operator(kind):
    for H, W, mapped in shape_cases(kind):
        c = stage_case("highlights", kind, H, W, mapped)
        if H * W >= 4096:
            raised = (c["ys"][0] > c["xs"][0]).mean()
            assert raised >= 0.02, f"highlights {kind} {H}x{W}: {raised} of the pixels rebuilt upward"


@pytest.mark.parametrize("kind", KINDS)
def test_chromatic_inputs_exercise_the_operator(kind):
    for H, W, mapped in shape_cases(kind):
        c = stage_case("chromatic", kind, H, W, mapped)
        if H * W >= 4096:
            rb = CR.red_blue(PATTERN[kind], H, W)
            changed = (c["ys"][0] != c["xs"][0])[rb].mean()
            assert changed >= 0.05, f"chromatic {kind} {H}x{W}: {changed} of the red / blue sites changed"
            assert np.array_equal(c["ys"][0][~rb], c["xs"][0][~rb])


@pytest.mark.parametrize("kind", KINDS)
def test_temporal_inputs_exercise_the_operator(kind):
    for H, W, mapped in shape_cases(kind):
        c = stage_case("temporal", kind, H, W, mapped)
        assert_exact(c["ys"][0], c["xs"][0], "an empty history gives y = x")
        if H * W >= 4096:
            same = (c["ys"][1] == c["xs"][1]).mean()
            assert same >= 0.10 and 1 - same >= 0.10, f"temporal {kind} {H}x{W}: {same} returned bit for bit"


@pytest.mark.parametrize("chain,kind", CHAIN_CASES)
def test_chain_inputs_exercise_every_stage(chain, kind):
    c = chain_case(chain, kind)
    for k, step in enumerate(c["steps"]):
        ins = step["inputs"]
        if "M" in chain:
            shares = M.classes(step["xs"], c["settings"]["M"], c["mask"])
            assert min(shares) >= 0.05, f"{chain} {kind} step {k}: the bracket does not exercise the merge {shares}"
        if "H" in chain:
            assert (step["ys"]["H"] > ins["H"]).mean() >= 0.02, f"{chain} {kind} step {k}: too few pixels rebuilt"
        if "C" in chain:
            rb = CR.red_blue(c["pattern"], *SEAMS)
            assert (step["ys"]["C"] != ins["C"])[rb].mean() >= 0.05, f"{chain} {kind} step {k}: chromatic changes too little"
        if "T" in chain and k == 1:
            assert (step["ys"]["T"] != ins["T"]).mean() >= 0.10, f"{chain} {kind}: the history does not matter"
        if "D" in chain:
            yg = D.route_yg(ins["D"], c["settings"]["D"], None, c["mask"])
            assert (np.abs(yg - ins["D"]) > 1e-4 * UNIT[kind]).mean() >= 0.10, f"{chain} {kind}: the filter changes too little"


# ---- 1. every (SRC, OUT) instance through the C ABI ---------------------------------------------------------------------
def raw_kind(kind):
    from taichi_image_amd import _native as N
    return {"p12": (N.MI_RAW_PACKED12, 0), "ids": (N.MI_RAW_PACKED12, 1), "p16": (N.MI_RAW_PACKED16, 0),
            "16u": (N.MI_RAW_16U, 0), "16f": (N.MI_RAW_16F, 0), "32f": (N.MI_RAW_32F, 0)}[kind]


def stage_args(c, kind, out, H, W, mapped, dev, keep):
    """(levels, shading, defects, work dtype code, plain, the output's torch dtype) of a C call; keep: what must outlive it."""
    from taichi_image_amd import _native as N
    plain = out == "plain"
    lv = N.levels_arg(c["black"], c["white"])
    g = to_dev(grid(), dev)
    arg = the_map(H, W)._arg(dev) if mapped else None
    keep += [lv, g, arg]
    # the plain form ignores the work dtype: both codes are passed across the kinds
    code = {"f16": N.MI_F16, "f32": N.MI_F32, "plain": N.MI_F16 if KINDS.index(kind) % 2 else N.MI_F32}[out]
    return lv, None if plain else N.shading_arg(g), arg, code, int(plain), torch.float16 if out == "f16" else torch.float32


@gpu
@pytest.mark.parametrize("stage,kind,out", STAGE_CASES)
def test_stage_instance(ti, dev, stage, kind, out):
    from taichi_image_amd import _native as N
    L, stream = N.lib(), N.stream_ptr(dev)
    mode, ids = raw_kind(kind)
    pattern = PATTERN[kind]
    for H, W, mapped in shape_cases(kind):
        c = stage_case(stage, kind, H, W, mapped)
        what = f"{stage} <{kind}, {out}> {H}x{W} map={mapped}"
        keep = []
        lv, sh, arg, code, plain, tdt = stage_args(c, kind, out, H, W, mapped, dev, keep)
        s = stage_settings(stage, kind, H, W)
        srcs = [to_dev(a, dev) for a in c["srcs"]]
        new = lambda dt=torch.float32: torch.full((H, W), -1.0, dtype=dt, device=dev)  # noqa: E731
        want = lambda y: y if plain else gained(y, out)  # noqa: E731
        if stage == "temporal":
            hin = None
            for k in range(2):
                hout, cfa = new(), None if plain else new(tdt)
                N.check(L.mi_isp_temporal_raw(srcs[k].data_ptr(), None if hin is None else hin.data_ptr(), hout.data_ptr(),
                                              None if plain else cfa.data_ptr(), H, W, mode, ids, code, lv, sh, arg, s._arg(),
                                              plain, stream))
                assert_exact(hout.cpu().numpy(), c["ys"][k], f"{what} step {k} history")
                if not plain:
                    assert_exact(cfa.cpu().numpy(), want(c["ys"][k]), f"{what} step {k} CFA")
                hin = hout
            continue
        dst = new(tdt)
        if stage == "merge":
            N.check(L.mi_isp_merge_raw(N.ptr_array(srcs), dst.data_ptr(), H, W, mode, ids, code, lv, sh, arg, s._arg(), plain,
                                       stream))
        elif stage == "highlights":
            N.check(L.mi_isp_highlights_raw(srcs[0].data_ptr(), dst.data_ptr(), H, W, mode, ids, code, pattern, lv, sh, arg,
                                            s._arg(WB), plain, stream))
        else:
            N.check(L.mi_isp_chromatic_raw(srcs[0].data_ptr(), dst.data_ptr(), H, W, mode, ids, code, pattern, lv, sh, arg,
                                           s._arg((H, W)), plain, stream))
        assert_exact(dst.cpu().numpy(), want(c["ys"][0]), what)


@gpu
@pytest.mark.parametrize("kind,work,radius", DENOISE_CASES)
def test_denoise_instance(ti, dev, kind, work, radius):
    from taichi_image_amd import _native as N
    L, stream = N.lib(), N.stream_ptr(dev)
    mode, ids = raw_kind(kind)
    for H, W, mapped in shape_cases(kind):
        c = stage_case("denoise", kind, H, W, mapped)
        keep = []
        lv, sh, arg, code, _, tdt = stage_args(c, kind, work, H, W, mapped, dev, keep)
        dn = stage_settings("denoise", kind, H, W, radius)
        src = to_dev(c["srcs"][0], dev)
        cfa = torch.full((H, W), -1.0, dtype=tdt, device=dev)
        p_maps = (ctypes.c_void_p * 1)(None if arg is None else ctypes.addressof(arg))
        N.check(L.mi_isp_denoise_raw_batch(N.ptr_array([src]), N.ptr_array([cfa]), 1, H, W, mode, ids, code, lv, sh, p_maps,
                                           dn._arg(), stream))
        listed = c["mask"] if mapped else np.zeros((H, W), bool)
        D.assert_within_bound(cfa.cpu().numpy(), D.route_yg(c["xs"][0], dn, pixel_gains(grid(), H, W), c["mask"]), work,
                              f"denoise <{kind}, {work}, R={radius}> {H}x{W} map={mapped}", where=~listed)


# ---- 2. every position of a stage in _raw_chain -------------------------------------------------------------------------
def chain_settings(chain, kind):
    H, W = SEAMS
    names = {"M": "merge", "H": "highlights", "C": "chromatic", "T": "temporal", "D": "denoise"}
    return {s: stage_settings(names[s], kind, H, W) for s in chain}


@functools.lru_cache(maxsize=None)
def chain_case(chain, kind):
    """The loads of a chain (two through one history when it has the temporal stage) and the references composed in
    _raw_chain's order: dict(steps=[dict(srcs, xs, inputs={stage: what it reads}, ys={stage: its y})], ...)."""
    H, W = SEAMS
    rng = _rng(50, list(CHAINS).index(chain), KINDS.index(kind))
    pattern = O.GRBG
    st = chain_settings(chain, kind)
    mask = the_mask(H, W)
    n = 2 if "T" in chain else 1
    if "M" in chain:                                       # a bracket per load: the same scene under fresh noise
        base = M.make_bracket(rng, H, W, RATIOS, GAIN, READ_NOISE)
        loads = [[np.clip(u + rng.normal(0, 1, u.shape) * M.noise_sigma(u, GAIN, READ_NOISE), 0, 1) for u in base]
                 for _ in range(n)]
    else:
        loads = [[u] for u in T.make_sequence(rng, H, W, n, GAIN, READ_NOISE)]
    if "H" in chain:                                       # clipped blobs in every frame
        lo = int(0.985 * 4095) + 1
        blobs = HR.make_codes(rng, H, W, 4095, lo, pattern) >= lo
        loads = [[np.where(blobs, 1.0, u) for u in us] for us in loads]
    steps, h, black, white = [], None, None, None
    for us in loads:
        enc = [encode(kind, u, levels=True) for u in us]
        black, white = enc[0][2], enc[0][3]
        xs = [e[1] for e in enc]
        y, inputs, ys = xs[0], {}, {}
        for s in chain:
            inputs[s] = y
            if s == "M":
                y = M.merge(xs, st["M"], mask)
            elif s == "H":
                y = HR.reconstruct(y, pattern, f32(WB), "rebuild", st["H"].clip, mask)
            elif s == "C":
                y = CR.correct(y, pattern, st["C"], mask)
            elif s == "T":
                y = h = T.blend(y, h, st["T"], mask)
            ys[s] = y                                      # (raw noise reduction: its input stands for it; the bound is its own)
        steps.append(dict(srcs=[_frozen(e[0]) for e in enc], xs=[_frozen(x) for x in xs],
                          inputs={s: _frozen(v) for s, v in inputs.items()}, ys={s: _frozen(v) for s, v in ys.items()}))
    return dict(steps=steps, settings=st, mask=mask, pattern=pattern, black=black, white=white)


def record_outputs(monkeypatch, name, index):
    """The tensors one library entry point wrote, cloned after every call (the probe of _count_calls, reading instead of
    counting): argument `index` is the pointer list _native.ptr_array made of them."""
    from taichi_image_amd import _native
    L = _native.lib()
    if not hasattr(_native.ptr_array, "lists"):
        orig = _native.ptr_array

        def ptr_array(tensors):
            arr = orig(tensors)
            ptr_array.lists[id(arr)] = (arr, list(tensors))  # (the array kept alive: its id stays its own)
            return arr
        ptr_array.lists = {}
        monkeypatch.setattr(_native, "ptr_array", ptr_array)
    fn, seen = getattr(L, name), []

    def recorded(*args):
        rc = fn(*args)
        seen.append([t.clone() for t in _native.ptr_array.lists[id(args[index])][1]])
        return rc
    monkeypatch.setattr(L, name, recorded)
    return seen


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("chain,kind", CHAIN_CASES)
def test_chain_positions(ti, dev, monkeypatch, cam, work, chain, kind):
    H, W = SEAMS
    c = chain_case(chain, kind)
    st, mask, pattern = c["settings"], c["mask"], c["pattern"]
    m = the_map(H, W)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, black_level=c["black"],
                           white_level=c["white"], lens_shading=np.array(grid()), exposure_merge=st.get("M"),
                           highlights=st.get("H"), chromatic_aberration=st.get("C"), temporal_denoise=st.get("T"),
                           raw_denoise=st.get("D"))
    wrote = {s: record_outputs(monkeypatch, *ENTRY[s]) for s in chain[:-1]}
    counts = {s: _count_calls(monkeypatch, ENTRY[s][0]) for s in "MHCTD"}
    got = capture(monkeypatch, isp)
    hist = ti.TemporalHistory() if "T" in chain else None
    kw = dict(defects=m) if hist is None else dict(defects=m, history=hist)
    for k, step in enumerate(c["steps"]):
        what = f"{cam} {chain} {kind} load {k}"
        got.clear()
        srcs = [to_dev(a, dev) for a in step["srcs"]]
        img = (load_bracket(isp, kind, srcs, **kw) if "M" in chain else call(isp, kind, srcs[0], **kw)).cpu().numpy()
        for s in chain[:-1]:                               # every stage in front of the last: its plain f32 y
            assert len(wrote[s]) == k + 1 and len(wrote[s][k]) == 1
            assert_exact(wrote[s][k][0].cpu().numpy(), step["ys"][s], f"{what}: the plain y of {s}")
        if hist is not None:
            assert hist.frames == k + 1
            assert_exact(hist.plane.cpu().numpy(), step["ys"]["T"], f"{what}: the temporal history")
        assert len(got) == 1
        cfa = got[0].cpu().numpy()
        if chain[-1] == "D":
            yg = D.route_yg(step["inputs"]["D"], st["D"], pixel_gains(grid(), H, W), mask)
            D.assert_within_bound(cfa, yg, work, what, where=~mask)
            assert_exact(cfa, correct_cfa(cfa, mask, work), what + ": the defect fix-up")
        else:
            assert_exact(cfa, cfa_of(isp, step["ys"][chain[-1]], work, mask), what + " CFA")
        check_image(isp, img, cfa, pattern, what)
    assert {s: len(n) for s, n in counts.items()} == {s: len(c["steps"]) if s in chain else 0 for s in "MHCTD"}


# ---- 3. the second launch of the batched entry points -------------------------------------------------------------------
SMALL = (6, 4)


def small_maps(ti, rng, n):
    """n different defect maps of a 6 x 4 frame."""
    H, W = SMALL
    out = []
    for k in range(n):
        sites = {(k % H, (k // H) % W), ((k + 3) % H, (k + 1) % W)} | {(int(rng.integers(H)), int(rng.integers(W)))}
        out.append(ti.DefectMap(sorted(sites), SMALL))
    return out


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
def test_temporal_batch_beyond_one_launch(ti, dev, monkeypatch, cam, work):
    """33 frames and histories, two steps, maps on frames 31 and 32: frame k is its own single load with its own history."""
    H, W = SMALL
    rng = _rng(60)
    kw = dict(device=dev, correct_colors=True, temporal_denoise=ti.TemporalDenoise(GAIN, READ_NOISE))
    a, b = getattr(ti, cam)(ti.BayerPattern.GRBG, **kw), getattr(ti, cam)(ti.BayerPattern.GRBG, **kw)
    seqs = [[to_dev(encode("p12", u)[0], dev) for u in T.make_sequence(rng, H, W, 2, GAIN, READ_NOISE)]
            for _ in range(N_TEMPORAL)]
    two = small_maps(ti, rng, 2)
    maps = [None] * 31 + two
    ha, hb = [ti.TemporalHistory() for _ in seqs], [ti.TemporalHistory() for _ in seqs]
    for step in range(2):
        n = _count_calls(monkeypatch, "mi_isp_temporal_raw_batch")
        imgs = a.load_packed12_batch([q[step] for q in seqs], defects=maps, history=ha)
        assert len(n) == 1
        for k in range(N_TEMPORAL):
            ref = b.load_packed12(seqs[k][step], defects=maps[k], history=hb[k])
            assert_exact(imgs[k].cpu().numpy(), ref.cpu().numpy(), f"{cam} step {step} frame {k} image")
            assert_exact(ha[k].plane.cpu().numpy(), hb[k].plane.cpu().numpy(), f"{cam} step {step} frame {k} history")
    planes = [h.plane.cpu().numpy() for h in ha]
    assert not np.array_equal(planes[0], planes[32]) and not np.array_equal(planes[1], planes[32])
    assert not any(np.array_equal(q[1].cpu().numpy(), q[0].cpu().numpy()) for q in seqs)


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("E", [3, 2])
def test_merge_batch_beyond_one_launch(ti, dev, monkeypatch, cam, work, E):
    """17 brackets, maps on brackets 15 and 16: each is its own single bracket load."""
    H, W = SMALL
    rng = _rng(61, E)
    ratios = {2: (1, 4), 3: RATIOS}[E]
    kw = dict(device=dev, correct_colors=True, exposure_merge=ti.ExposureMerge(ratios, GAIN, READ_NOISE, saturation=0.9))
    a, b = getattr(ti, cam)(ti.BayerPattern.GBRG, **kw), getattr(ti, cam)(ti.BayerPattern.GBRG, **kw)
    brackets = [[to_dev(f, dev) for f in bracket(rng, "p12", H, W, E)[0]] for _ in range(N_MERGE)]
    maps = [None] * 15 + small_maps(ti, rng, 2)
    n = _count_calls(monkeypatch, "mi_isp_merge_raw_batch")
    imgs = a.load_packed12_bracket_batch(brackets, defects=maps)
    assert len(n) == 1
    singles = [b.load_packed12_bracket(brackets[k], defects=maps[k]).cpu().numpy() for k in range(N_MERGE)]
    for k in range(N_MERGE):
        assert_exact(imgs[k].cpu().numpy(), singles[k], f"{cam} E={E} bracket {k}")
    assert len({s.tobytes() for s in singles}) == N_MERGE, "every bracket has content of its own"
    # ... and a frame of another bracket in a bracket's place changes the image (the index into the table matters)
    swapped = b.load_packed12_bracket([brackets[16][0]] + brackets[15][1:]).cpu().numpy()
    assert not np.array_equal(swapped, singles[16])


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
def test_awb_statistics_beyond_one_launch(ti, dev, cam, work):
    """33 frames in one batch load: the pending sums are the exact integer sums of 33 single loads on fresh cameras."""
    H, W = SMALL
    rng = _rng(62)
    frames = [to_dev(encode("p12", 0.1 + 0.8 * rng.random((H, W)))[0], dev) for _ in range(N_AWB)]
    new = lambda: getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, correct_colors=True, auto_white_balance=True)  # noqa: E731
    isp = new()
    isp.load_packed12_batch(frames)
    singles = []
    for f in frames:
        one = new()
        one.load_packed12(f)
        singles.append(one._awb_pending.cpu().numpy().view(np.uint64))
    assert all(s.any() for s in singles) and not np.array_equal(singles[0], singles[32])
    assert not np.array_equal(singles[0] + singles[31], singles[31] + singles[32])
    total = np.sum(np.stack(singles), axis=0, dtype=np.uint64)
    assert_exact(isp._awb_pending.cpu().numpy().view(np.uint64), total, f"{cam} pending sums of {N_AWB} frames")


def lens_borders(last):
    """The border modes of the 35 frames: 33 constant and 2 replicate, the last frame `last`."""
    replicate = {5, 20} if last == "constant" else {5, N_LENS - 1}
    return ["replicate" if i in replicate else "constant" for i in range(N_LENS)]


@gpu
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("last", ["constant", "replicate"])
def test_undistort_batch_beyond_one_launch(ti, dev, dt, last):
    """mi_isp_undistort_batch with 35 frames in two border buckets that flush independently: each output is
    mi_isp_undistort of that frame."""
    from taichi_image_amd import _native as N
    L, stream = N.lib(), N.stream_ptr(dev)
    H, W = SMALL
    rng = _rng(63)
    code = N.MI_F16 if dt == "f16" else N.MI_F32
    tdt = torch.float16 if dt == "f16" else torch.float32
    lenses = []
    for i, border in enumerate(lens_borders(last)):
        K = np.array([[0.62 * W + 0.01 * i, 0.0, W / 2 - 0.37], [0.0, 0.6 * W, H / 2 + 0.21 - 0.01 * i], [0.0, 0.0, 1.0]])
        wide = K * np.array([[0.8], [0.82], [1.0]])          # (the corners sample outside the source: the border rule)
        lenses.append(ti.LensDistortion(K, (-0.32, 0.11, 0.004, -0.0025), (H, W), new_K=wide, border=border))
    srcs = [(0.1 + rng.random((H, W, 3), dtype=f32)).astype(O.NP_DTYPE[dt]) for _ in range(N_LENS)]
    ts = [to_dev(s, dev) for s in srcs]
    args = [m._arg() for m in lenses]
    singles = []
    for t, a in zip(ts, args):
        out = torch.full((H, W, 3), -1.0, dtype=tdt, device=dev)
        N.check(L.mi_isp_undistort(t.data_ptr(), out.data_ptr(), H, W, H, W, 1.0, 1.0, code, code, a, stream))
        singles.append(out.cpu().numpy())
    outs = [torch.full((H, W, 3), -1.0, dtype=tdt, device=dev) for _ in range(N_LENS)]
    p_lens = (ctypes.c_void_p * N_LENS)(*[ctypes.addressof(a) for a in args])
    N.check(L.mi_isp_undistort_batch(N.ptr_array(ts), N.ptr_array(outs), N_LENS, H, W, H, W, 1.0, 1.0, code, code, p_lens,
                                     stream))
    for i in range(N_LENS):
        assert_exact(outs[i].cpu().numpy(), singles[i], f"{dt} frame {i} ({lenses[i].border})")
    assert len({s.tobytes() for s in singles}) == N_LENS, "every frame has an output of its own"
    # the border mode shows in the outputs: the same frame under the other mode differs
    other = ti.LensDistortion(lenses[5].K, lenses[5].dist, (H, W), new_K=lenses[5].new_K, border="constant")
    out = torch.full((H, W, 3), -1.0, dtype=tdt, device=dev)
    N.check(L.mi_isp_undistort(ts[5].data_ptr(), out.data_ptr(), H, W, H, W, 1.0, 1.0, code, code, other._arg(), stream))
    assert not np.array_equal(out.cpu().numpy(), singles[5])


def defect_slots(last_mapped):
    """Which of the 36 frames has a map: 33 of them; none at index 0 and at index 10, and either none at the last index or
    none at index 20."""
    none = {0, 10, 20 if last_mapped else N_DEFECTS - 1}
    return [i not in none for i in range(N_DEFECTS)]


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("last_mapped", [False, True])
def test_defect_fix_up_beyond_one_launch(ti, dev, monkeypatch, cam, work, last_mapped):
    """36 frames, 33 of them with a map of their own: each image is its single load."""
    H, W = SMALL
    rng = _rng(64, last_mapped)
    isp = getattr(ti, cam)(ti.BayerPattern.BGGR, device=dev, correct_colors=True)
    frames = [to_dev(encode("p12", 0.05 + 0.9 * rng.random((H, W)))[0], dev) for _ in range(N_DEFECTS)]
    own = iter(small_maps(ti, rng, N_MAPPED))
    maps = [next(own) if slot else None for slot in defect_slots(last_mapped)]
    n = _count_calls(monkeypatch, "mi_isp_defects_fix_packed_batch")
    imgs = isp.load_packed12_batch(frames, defects=maps)
    assert len(n) == 1
    for k in range(N_DEFECTS):
        single = isp.load_packed12(frames[k], defects=maps[k]).cpu().numpy()
        assert_exact(imgs[k].cpu().numpy(), single, f"{cam} frame {k} (map: {maps[k] is not None})")
        if maps[k] is not None:
            assert not np.array_equal(single, isp.load_packed12(frames[k]).cpu().numpy()), f"frame {k}: the map shows"


# ---- 4. the alignment forks ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("out", OUTS)
def test_merge_narrow_store_on_an_even_width(ti, dev, out):
    """W even, the destination one element off: the narrow route.  The result is the aligned call's (and the reference's),
    and nothing around the view is written."""
    from taichi_image_amd import _native as N
    L, stream = N.lib(), N.stream_ptr(dev)
    H, W = SEAMS
    kind = "16u"
    c = stage_case("merge", kind, H, W, True)
    keep = []
    lv, sh, arg, code, plain, tdt = stage_args(c, kind, out, H, W, True, dev, keep)
    s = stage_settings("merge", kind, H, W)
    mode, ids = raw_kind(kind)
    srcs = [to_dev(a, dev) for a in c["srcs"]]
    aligned = torch.full((H, W), -7.0, dtype=tdt, device=dev)
    whole = torch.full((H * W + 9,), -7.0, dtype=tdt, device=dev)
    view = whole[1:1 + H * W].view(H, W)
    size = whole.element_size()
    assert aligned.data_ptr() % (2 * size) == 0 and view.data_ptr() % (2 * size) == size and view.is_contiguous()
    for dst in (aligned, view):
        N.check(L.mi_isp_merge_raw(N.ptr_array(srcs), dst.data_ptr(), H, W, mode, ids, code, lv, sh, arg, s._arg(), plain,
                                   stream))
    assert_exact(aligned.cpu().numpy(), c["ys"][0] if plain else gained(c["ys"][0], out), f"{out} aligned")
    assert_exact(view.cpu().numpy(), aligned.cpu().numpy(), f"{out} one element off")
    around = torch.cat([whole[:1], whole[1 + H * W:]]).cpu().numpy()
    assert_exact(around, np.full(9, -7.0, around.dtype), f"{out}: the elements around the view")


@gpu
@pytest.mark.parametrize("work", ["f16", "f32"])
def test_local_tonemap_on_an_image_one_element_off(ti, dev, work):
    """W % 4 == 0, the image one element off its allocation: the element-wise route, the reference's bits."""
    from taichi_image_amd import local_tonemap as ltm
    H, W, kw = 24, 40, dict(cell=8, bins=32, strength=0.8)
    dtype = np.float16 if work == "f16" else np.float32
    img = LR.make_image(_rng(70), H, W, "wide", dtype)
    want = LR.local_tonemap(img, kw)
    assert not np.array_equal(want, img)
    n = H * W * 3
    whole = torch.full((n + 9,), -7.0, dtype=torch.float16 if work == "f16" else torch.float32, device=dev)
    view = whole[1:1 + n].view(H, W, 3)
    view.copy_(torch.from_numpy(img))
    assert W % 4 == 0 and view.data_ptr() % 16 == whole.element_size() and view.is_contiguous()
    ltm.apply([view], ti.LocalTonemap(**kw))
    assert_exact(view.cpu().numpy(), want, f"{work} one element off")
    around = torch.cat([whole[:1], whole[1 + n:]]).cpu().numpy()
    assert_exact(around, np.full(9, -7.0, around.dtype), f"{work}: the elements around the view")
