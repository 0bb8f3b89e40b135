"""The multi-pass chain (`pipeline12_reinhard(..., whole_frame=False)`, csrc/isp_api.hip: pipeline12_frame) route by
route.  Behind its one entry point it is four chains of kernels (include/mi_isp.h, mi_isp_pipeline12_route):

  stream          strm::stream_kernel<E, PR, PC, S_BOUNDS / S_STATS / S_RH_MINMAX / S_RH_STORE>
  cached_stream   stream_kernel<.., S_STORE_BOUNDS>, then three ew::tonemap_reinhard_tail passes
  cached_tile     tile::tile_kernel<.., EPI_STORE_MINMAX, HOT 0 or 1>, then the tails
  recompute       tile_kernel<.., EPI_MINMAX / EPI_STATS / EPI_RH_MINMAX / EPI_RH_STORE> and three ew::finalize launches

Every GPU case asks the library which route its ACTUAL pointers take (the query is the function the launches go through)
and, on the stream routes, how many rows a wave gets, and asserts both before it compares anything.

The stream kernel's body is unrolled in three rotations of a 3-slot raw-row ring and a 6-row window ring.  A wave of
rows_per_wave rows runs rows_per_wave / 2 row pairs; the frames of the rest of the suite below 2448 x 2050 all give 2:

  pairs  first to reach                                                       frames here (H, W) -> rows in the last band
  2      the prologue's loads cover everything (the control)                   (26, 520) -> 2
  3      rotation 2 live, one exact turn of the ring                           (8200, 16) -> 4; (4100, 520), two bands -> 2;
                                                                               (3074, 1032), three bands -> 2
  4      a row consumed that was loaded inside the loop; dead rotations 1, 2   (12290, 16) -> 2; (6146, 520) -> 2;
                                                                               (12290, 8): one lane that is both borders
  5      a turn and two thirds                                                 (16396, 16) -> 6
  6      two exact turns (what 4096 x 3072 runs)                               (20482, 16) -> 10

The classes are read from the query, so a change of strm::geometry's target fails the no-GPU test below, which names
the shapes to move.  Every instance (4 CFA patterns x f16 / f32 work dtype) runs every shape; the runtime branches
(gamma 1 / 0.5 / 0.6, color_adapt, the colour matrix, bounds exactly (0, 1) or inside) and the output dtype come from the
shape's index (branches(), out_dtype()).  The reference is the C oracle, or the NumPy oracle where the C oracle has no
counterpart (the colour matrix, u16 outputs), at the parity contract of tests/util.assert_close with its defaults; a
second launch gives the same bits.

The S_STORE loaders (load_packed12, metered and plain; load_packed12_batch of 10 frames) run on a 3-, a 4- and a 5-pair
frame for Camera16 / Camera32 x 4 patterns x the four levels modes, bit for bit against tests/test_gpu_shading.ref_load,
the tagged stride-8 subsample included.

Not here: rstrm::resize_kernel's ring at more rows per wave (tests/test_gpu_resize_bands.py covers its seams; its ring
classes are a follow-up); the whole-frame and camera-group kernels have their own files.

The first tests need no GPU: the route query on made-up addresses gives the table of include/mi_isp.h; the shapes have
the classes claimed; every instance meets both sides of every branch; and - on the oracle alone - every reference is
finite, "unit" frames have demosaiced bounds exactly (0, 1), "non-unit" frames lie strictly inside, and the side of each
colour-matrix case is the one recorded in CCM_BOUNDS."""
import functools

import numpy as np
import pytest

from oracle import c_oracle, isp_oracle as O
from tests.test_gpu_shading import PER_SITE, make_grid, ref_load
from tests.test_gpu_whole_frame_pairs import frame as pairs_frame
from tests.util import assert_close, assert_exact

pytestmark = pytest.mark.skipif(not c_oracle.available(), reason="oracle/liborc_isp.so not built")

PATTERNS = {"RGGB": O.RGGB, "GRBG": O.GRBG, "GBRG": O.GBRG, "BGGR": O.BGGR}
WORKS = ["f16", "f32"]
INSTANCES = [(p, w) for p in PATTERNS for w in WORKS]
OUTS = {"f16": ["f16", "u8", "u16"], "f32": ["f32", "u8"]}            # the stream cases' output dtypes per work dtype
CODE = {"u8": 0, "u16": 1, "f16": 2, "f32": 3}                         # MI_U8 .. MI_F32
SIZE = {"u8": 1, "u16": 2, "f16": 2, "f32": 4}
CCM = O.isp_color_matrix(True, O.DEFAULT_WB, O.DEFAULT_CC)

# (H, W) -> (pairs, rows in the last band, column bands); (12290, 8) last: its index has the "unit" bit clear (the two
# patches of a unit frame do not fit 8 columns)
STREAM_SHAPES = [(26, 520), (8200, 16), (4100, 520), (3074, 1032), (12290, 16), (6146, 520), (16396, 16), (20482, 16),
                 (12290, 8)]
STREAM_CLASS = {(26, 520): (2, 2, 2), (8200, 16): (3, 4, 1), (4100, 520): (3, 2, 2), (3074, 1032): (3, 2, 3),
                (12290, 16): (4, 2, 1), (6146, 520): (4, 2, 2), (16396, 16): (5, 6, 1), (20482, 16): (6, 10, 1),
                (12290, 8): (4, 2, 1)}
TILE_SHAPES = [(32, 128), (34, 136), (70, 264)]                        # ragged right and bottom tiles around 128 x 32
RAGGED_SHAPES = [(34, 130), (70, 266)]                                 # W % 8 == 2

# With the colour matrix the demosaiced bounds are what the matrix and the clamp make of them.  Recorded from the oracle
# (test_colour_matrix_cases_fall_on_the_recorded_side): a unit frame stays at exactly (0, 1); a non-unit frame's top
# clamps to exactly 1 while its bottom stays above 0, so it stays on the non-unit side - lo > 0, hi == 1.
CCM_BOUNDS = {True: "lo == 0 and hi == 1", False: "0 < lo < 0.5 and hi == 1"}


def branches(i):
    """The runtime branches of case i of a list, from the bits of its index: gamma by i % 3 (1.0 skips the pow, 0.5 is an
    integral 1 / gamma, 0.6 a fractional one), color_adapt != 0 by bit 0 (with an intensity and a light_adapt to go with
    it), the colour matrix by bit 1 (light_adapt < 1 there: a pixel the matrix clamps to black stays finite), bounds
    exactly (0, 1) by bit 2.  Returns (kw, ccm on, unit)."""
    kw = dict(gamma=(1.0, 0.5, 0.6)[i % 3], intensity=1.0, light_adapt=1.0, color_adapt=0.0)
    if i & 1:
        kw.update(intensity=1.5, light_adapt=0.7, color_adapt=0.4)
    elif i & 2:
        kw.update(light_adapt=0.8)
    return kw, bool(i & 2), bool(i & 4)


def out_dtype(i, pattern, work):
    """The output dtype of stream case i: over the shapes every pattern stores through every arm of S_RH_STORE's switch."""
    outs = OUTS[work]
    return outs[(i + PATTERNS[pattern]) % len(outs)]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def packed_frame(shape, pattern, unit, ids=False):
    """tests/test_gpu_whole_frame_pairs.frame; ids: the same codes in the IDS layout."""
    packed = pairs_frame(shape[0], shape[1], PATTERNS[pattern], unit)
    if ids:
        packed = O.encode12(O.decode12(packed, "u16"), ids_format=True)
    return _frozen(packed)


@functools.lru_cache(maxsize=64)
def reference(shape, pattern, work, out, i, ids=False):
    """The oracle's pipeline12_reinhard of case i's frame (computed once per case, read-only)."""
    kw, ccm, unit = branches(i)
    packed = packed_frame(shape, pattern, unit, ids)
    if ccm or out == "u16":                                 # the C oracle has neither
        return _frozen(O.pipeline12_reinhard(packed, PATTERNS[pattern], ids, CCM if ccm else None, work, out, **kw))
    return _frozen(c_oracle.pipeline12_reinhard(packed, pattern=PATTERNS[pattern], ids=ids, work=work, out=out, **kw))


def demosaiced_bounds(shape, pattern, work, unit, ccm):
    H, W = shape
    cfa = c_oracle.decode12_scaled(packed_frame(shape, pattern, unit), work=work).reshape(H, W)
    rgb = np.clip(c_oracle.demosaic(cfa, PATTERNS[pattern], ccm=CCM if ccm else None, round_f16=work == "f16"), 0.0, 1.0)
    return float(rgb.min()), float(rgb.max())


def fake_route(packed, out, work_image, H, W, ids, work, odt):
    from taichi_image_amd import _native
    return _native.pipeline12_route(packed, out, work_image, H, W, ids, CODE[work], CODE[odt])


# ---------------------------------------------------------------------------------------------------------------------
# preconditions (no GPU)

A = 0x7F0000000000                                          # made-up addresses: the query never dereferences


@pytest.mark.parametrize("work", WORKS)
@pytest.mark.parametrize("odt", ["u8", "u16", "f16", "f32"])
def test_route_query_gives_the_table(work, odt):
    """mi_isp_pipeline12_route on fabricated addresses: both layouts, W % 8 of 0 and 2, H of 2 and 4, aligned and
    misaligned packed / out / work image, every work / out pair."""
    same = work == odt
    out_align = 8 if odt == "u8" else 16
    out_off = SIZE[odt]                                     # the smallest offset a view of that dtype can have
    img_off = SIZE[work]
    OUT, IMG = A + (1 << 30), A + (2 << 30)
    for H in (2, 4):
        for W in (16, 18, 136, 138, 520):
            for ids in (0, 1):
                for p_off in (0, 1, 4):
                    for o_off in (0, out_off, out_align):
                        for image in (None, IMG, IMG + img_off):
                            name, r = fake_route(A + p_off, OUT + o_off, image, H, W, ids, work, odt)
                            what = f"H {H} W {W} ids {ids} packed +{p_off} out +{o_off} image {image and image - IMG}"
                            strm = not ids and H >= 4 and W % 8 == 0 and p_off % 4 == 0
                            out_ok = W % 8 == 0 and o_off % out_align == 0
                            img_ok = out_ok if same else (W % 8 == 0 and image == IMG)
                            if strm and out_ok:
                                want = "stream"
                            elif img_ok:
                                want = "cached_stream" if strm else "cached_tile"
                            else:
                                want = "recompute"
                            assert name == want, what
                            assert r.hot == (1 if want == "cached_tile" and p_off % 4 == 0 else 0), what
                            if want in ("stream", "cached_stream"):
                                assert r.rows_per_wave == 4 and r.bands_x == -(-W // 512), what
                                assert r.n_blocks == -(-(r.bands_x * -(-H // 4)) // 4), what
                            else:
                                assert r.rows_per_wave == 0 and r.bands_x == 0, what
                                assert r.n_blocks == -(-W // 128) * -(-H // 32), what


def test_route_query_refuses_what_the_chain_refuses():
    from taichi_image_amd import _native
    L = _native.lib()
    r = _native.Route()
    assert L.mi_isp_pipeline12_route(None, A, None, 4, 16, 0, 2, 2, r) != 0 and b"null" in L.mi_isp_last_error()
    assert L.mi_isp_pipeline12_route(A, None, None, 4, 16, 0, 2, 2, r) != 0
    assert L.mi_isp_pipeline12_route(A, A, None, 3, 16, 0, 2, 2, r) != 0 and b"even" in L.mi_isp_last_error()
    assert L.mi_isp_pipeline12_route(A, A, None, 4, 16, 0, 0, 2, r) != 0 and b"work dtype" in L.mi_isp_last_error()
    assert L.mi_isp_pipeline12_route(A, A, None, 4, 16, 0, 2, 9, r) != 0
    assert L.mi_isp_pipeline12_route(A, A, None, 4, 16, 0, 2, 2, None) != 0


def test_stream_shapes_have_the_ring_classes_claimed():
    """Read from the query, not from a restated formula: if strm::geometry changes, these are the shapes to move."""
    assert set(STREAM_SHAPES) == set(STREAM_CLASS) and len(STREAM_SHAPES) == len(STREAM_CLASS)
    for shape in STREAM_SHAPES:
        H, W = shape
        for work in WORKS:
            for odt in OUTS[work]:
                name, r = fake_route(A, A + (1 << 30), None, H, W, 0, work, odt)
                assert name == "stream", (shape, work, odt)
                last = H - (-(-H // r.rows_per_wave) - 1) * r.rows_per_wave
                assert (r.rows_per_wave // 2, last, r.bands_x) == STREAM_CLASS[shape], \
                    f"{shape}: {r.rows_per_wave} rows per wave, {last} in the last band, {r.bands_x} column bands"
                assert r.rows_per_wave % 2 == 0 and r.n_blocks == -(-(r.bands_x * -(-H // r.rows_per_wave)) // 4)
    pairs = [STREAM_CLASS[s][0] for s in STREAM_SHAPES]
    assert set(pairs) == {2, 3, 4, 5, 6} and pairs.count(2) == 1, "every ring class; one control"
    last_pairs = {STREAM_CLASS[s][1] // 2 for s in STREAM_SHAPES}
    assert 1 in last_pairs and 2 in last_pairs and any(n > 3 for n in last_pairs), \
        "last bands of 1 pair, of 2 pairs and of more than one turn of the ring"
    assert {STREAM_CLASS[s][2] for s in STREAM_SHAPES if STREAM_CLASS[s][0] == 3} == {1, 2, 3}
    assert any(STREAM_CLASS[s][0] == 4 and STREAM_CLASS[s][2] == 2 for s in STREAM_SHAPES)
    assert (12290, 8) in STREAM_SHAPES, "one lane that is both borders"
    for shape in LOADER_SHAPES + CACHED_STREAM_SHAPES:
        assert shape in STREAM_CLASS
    assert [STREAM_CLASS[s][0] for s in LOADER_SHAPES] == [3, 4, 5] and STREAM_CLASS[LOADER_SHAPES[0]][2] == 2
    assert [STREAM_CLASS[s][0] for s in CACHED_STREAM_SHAPES] == [2, 4]
    assert (32, 128) in TILE_SHAPES and all(W % 8 == 0 for _, W in TILE_SHAPES), "one exact tile; whole strips"
    assert any(H % 32 and W % 128 for H, W in TILE_SHAPES), "ragged bottom and right tiles"
    assert {c[1] for c in CACHED_TILE_CASES} == set(TILE_SHAPES)
    assert {c[1] for c in RECOMPUTE_CASES} == set(TILE_SHAPES) | set(RAGGED_SHAPES)
    assert all(W % 8 == 2 for _, W in RAGGED_SHAPES)


def _sides(cases):
    """The sides of each branch a list of case indices meets."""
    seen = [branches(i) for i in cases]
    return ({kw["gamma"] for kw, _, _ in seen}, {kw["color_adapt"] != 0.0 for kw, _, _ in seen},
            {c for _, c, _ in seen}, {u for _, _, u in seen})


BOTH = ({1.0, 0.5, 0.6}, {False, True}, {False, True}, {False, True})


def test_every_instance_meets_both_sides_of_every_branch():
    """Every instance runs every case of a list, so these are properties of the lists alone."""
    assert len(INSTANCES) == 8 and len(set(INSTANCES)) == 8
    n = len(STREAM_SHAPES)
    assert _sides(range(n)) == BOTH
    assert _sides([i for i in range(n) if STREAM_CLASS[STREAM_SHAPES[i]][0] >= 3]) == BOTH, "and beyond the control"
    assert not branches(STREAM_SHAPES.index((12290, 8)))[2], "no unit frame at W = 8"
    for pattern, work in INSTANCES:
        assert {out_dtype(i, pattern, work) for i in range(n)} == set(OUTS[work])
        assert {out_dtype(i, pattern, work) for i in range(n) if STREAM_CLASS[STREAM_SHAPES[i]][0] >= 3} == set(OUTS[work])
    for kw, ccm, _ in map(branches, range(16)):
        assert not ccm or kw["light_adapt"] < 1.0
    assert _sides(range(len(RECOMPUTE_CASES))) == BOTH
    for kind in ("work", "u8", "u16"):
        mine = [i for i, c in enumerate(RECOMPUTE_CASES) if c[2] == kind]
        g, ca, cc, un = _sides(mine)
        assert (ca, cc, un) == BOTH[1:], f"recompute cases with output {kind}"
    assert {c[0] for c in RECOMPUTE_CASES} == {"ids", "off1", "ragged", "outview"}
    assert {(c[0], c[2]) for c in CACHED_TILE_CASES} >= {("ids", "u8"), ("ids", "work"), ("off1", "u8"), ("off1", "work")}
    assert _sides(range(len(CACHED_TILE_CASES)))[1:] == BOTH[1:]
    assert _sides(CACHED_STREAM_BRANCH)[1:] == BOTH[1:]


@pytest.mark.parametrize("pattern,work", INSTANCES)
def test_frames_have_the_bounds_the_gpu_cases_assume(pattern, work):
    """On the oracle alone, without the colour matrix: unit frames have demosaiced bounds exactly (0, 1), the others lie
    strictly inside; every stream reference is finite."""
    for i, shape in enumerate(STREAM_SHAPES):
        kw, ccm, unit = branches(i)
        if not ccm:
            lo, hi = demosaiced_bounds(shape, pattern, work, unit, False)
            assert ((lo, hi) == (0.0, 1.0)) if unit else (0.0 < lo < hi < 1.0), f"{shape} {pattern} {work}: {lo} .. {hi}"
        ref = reference(shape, pattern, work, out_dtype(i, pattern, work), i)
        assert ref.shape == shape + (3,) and np.isfinite(ref.astype(np.float32)).all(), f"{shape} {pattern} {work}"


@pytest.mark.parametrize("pattern,work", INSTANCES)
def test_tile_frames_have_the_bounds_the_gpu_cases_assume(pattern, work):
    for cases in (RECOMPUTE_CASES, CACHED_TILE_CASES):
        for i, (way, shape, kind) in enumerate(cases):
            kw, ccm, unit = branches(i)
            if not ccm:
                lo, hi = demosaiced_bounds(shape, pattern, work, unit, False)
                assert ((lo, hi) == (0.0, 1.0)) if unit else (0.0 < lo < hi < 1.0), f"{shape} {pattern} {work}: {lo} .. {hi}"
            out = work if kind == "work" else kind
            ref = reference(shape, pattern, work, out, i, way == "ids")
            assert np.isfinite(ref.astype(np.float32)).all(), f"{way} {shape} {pattern} {work}"


@pytest.mark.parametrize("pattern,work", INSTANCES)
def test_colour_matrix_cases_fall_on_the_recorded_side(pattern, work):
    """With the matrix the clamp decides the bounds: every colour-matrix case falls on the side CCM_BOUNDS records for
    its kind of frame, so the unit bit of branches() still says which side of the bounds branch a case runs."""
    for cases in ([("", s, "") for s in STREAM_SHAPES], RECOMPUTE_CASES, CACHED_TILE_CASES,
                  [("", s, "") for s in CACHED_STREAM_SHAPES]):
        for i, (_, shape, _) in enumerate(cases):
            if cases[0][1] == CACHED_STREAM_SHAPES[0] and len(cases) == len(CACHED_STREAM_SHAPES):
                i = CACHED_STREAM_BRANCH[i]
            kw, ccm, unit = branches(i)
            if ccm:
                lo, hi = demosaiced_bounds(shape, pattern, work, unit, True)
                assert eval(CCM_BOUNDS[unit], dict(lo=lo, hi=hi)), f"{shape} {pattern} {work} unit {unit}: {lo} .. {hi}"


# ---------------------------------------------------------------------------------------------------------------------
# GPU side

@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def _torch_dtype(name):
    import torch
    return {"u8": torch.uint8, "u16": torch.uint16, "f16": torch.float16, "f32": torch.float32}[name]


def _view_at(dev, shape, dtype_name, offset):
    """A contiguous tensor of that shape and dtype whose first byte lies `offset` bytes into a fresh (aligned) buffer."""
    import torch
    n = int(np.prod(shape)) * SIZE[dtype_name]
    buf = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    t = buf[offset:offset + n].view(_torch_dtype(dtype_name)).view(*shape)
    assert t.data_ptr() == buf.data_ptr() + offset and t.is_contiguous()
    return t


def _packed_at(dev, packed, offset):
    import torch
    t = _view_at(dev, packed.shape, "u8", offset)
    t.copy_(torch.from_numpy(np.array(packed)))
    return t


def run_chain(ti, dev, src, out, work_image, shape, pattern, ids, work, odt, ccm, kw, want_route, want_hot=0, want_rpw=None):
    """mi_isp_pipeline12_reinhard on exactly these buffers, twice: asserts the route of the actual pointers first, and
    that the second launch gives the first one's bits.  Returns the output on the host."""
    import torch
    from taichi_image_amd import _native
    H, W = shape
    wi = None if work_image is None else work_image.data_ptr()
    name, r = _native.pipeline12_route(src.data_ptr(), out.data_ptr(), wi, H, W, ids, CODE[work], CODE[odt])
    assert name == want_route, f"route {name}, the case was written for {want_route}"
    assert r.hot == want_hot, f"first pass HOT {r.hot}, the case was written for {want_hot}"
    if want_rpw is not None:
        assert r.rows_per_wave == want_rpw, f"{r.rows_per_wave} rows per wave, the case was written for {want_rpw}"
    ws = _native.workspace(H, W, dev)
    got = []
    for rep in range(2):
        out.zero_()
        _native.check(_native.lib().mi_isp_pipeline12_reinhard(
            src.data_ptr(), out.data_ptr(), wi, H, W, int(ids), PATTERNS[pattern], _native.ccm_arg(CCM if ccm else None),
            CODE[work], CODE[odt], kw["gamma"], kw["intensity"], kw["light_adapt"], kw["color_adapt"], ws.data_ptr(),
            _native.stream_ptr(dev)))
        torch.cuda.synchronize()
        got.append(out.cpu().numpy())
    assert_exact(got[1], got[0], "second launch")
    return got[0]


def stream_id(v):
    if isinstance(v, tuple):
        i = STREAM_SHAPES.index(v)
        kw, ccm, unit = branches(i)
        return (f"{v[0]}x{v[1]}-{STREAM_CLASS[v][0]}pairs-g{kw['gamma']}-ca{kw['color_adapt']}-{'ccm' if ccm else 'noccm'}-"
                f"{'unit' if unit else 'nonunit'}")
    return str(v)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=stream_id)
@pytest.mark.parametrize("pattern,work", INSTANCES)
def test_stream_route_at_every_ring_class(ti, dev, pattern, work, shape):
    """Route "stream": one instance at one ring class, through the Python entry point with whole_frame=False."""
    import torch
    from taichi_image_amd import _native
    from taichi_image_amd.pipeline import pipeline12_reinhard
    i = STREAM_SHAPES.index(shape)
    kw, ccm, unit = branches(i)
    odt = out_dtype(i, pattern, work)
    what = f"stream {pattern} {work}->{odt} {stream_id(shape)}"
    H, W = shape
    src = torch.from_numpy(np.array(packed_frame(shape, pattern, unit))).to(dev)
    out = torch.empty((H, W, 3), dtype=_torch_dtype(odt), device=dev)
    for image in (None, A):                                  # (the Python wrapper brings an aligned work image along)
        name, r = _native.pipeline12_route(src.data_ptr(), out.data_ptr(), image, H, W, 0, CODE[work], CODE[odt])
        assert name == "stream" and r.rows_per_wave == 2 * STREAM_CLASS[shape][0] and r.bands_x == STREAM_CLASS[shape][2], what
    got = []
    for rep in range(2):
        out.zero_()
        res = pipeline12_reinhard(src, pattern=ti.BayerPattern(PATTERNS[pattern]), correct_colors=CCM if ccm else None,
                                  work_dtype=work, dtype=odt, out=out, whole_frame=False, **kw)
        torch.cuda.synchronize()
        assert res is out
        got.append(out.cpu().numpy())
    assert_close(got[0], reference(shape, pattern, work, odt, i), what)
    assert_exact(got[1], got[0], what + ": second launch")


CACHED_STREAM_SHAPES = [(26, 520), (12290, 16)]
# branches(): ca 0.4, no matrix, non-unit (a stale or missing partial result of the bounds then shows: lo is not 0);
# ca 0, the matrix, unit
CACHED_STREAM_BRANCH = [1, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CACHED_STREAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pattern,work", INSTANCES)
def test_cached_route_stream_first_pass(ti, dev, pattern, work, shape):
    """Route "cached_stream" (S_STORE_BOUNDS + the tails): a u8 output that is a view 4 bytes into a larger buffer, with
    an aligned work image, at a 2-pair and a 4-pair shape."""
    i = CACHED_STREAM_BRANCH[CACHED_STREAM_SHAPES.index(shape)]
    kw, ccm, unit = branches(i)
    what = f"cached_stream {pattern} {work}->u8 {shape} {kw} ccm {ccm} unit {unit}"
    src = _packed_at(dev, packed_frame(shape, pattern, unit), 0)
    out = _view_at(dev, shape + (3,), "u8", 4)
    image = _view_at(dev, shape + (3,), work, 0)
    got = run_chain(ti, dev, src, out, image, shape, pattern, 0, work, "u8", ccm, kw, "cached_stream",
                    want_rpw=2 * STREAM_CLASS[shape][0])
    assert_close(got, reference(shape, pattern, work, "u8", i), what)


# (way, shape, output): "ids" an IDS frame (HOT 1), "off1" a standard frame one byte off its 4-byte boundary (HOT 0)
CACHED_TILE_CASES = [("ids", (32, 128), "u8"), ("ids", (34, 136), "work"), ("ids", (70, 264), "u16"),
                     ("off1", (32, 128), "work"), ("off1", (34, 136), "u8"), ("off1", (70, 264), "work"),
                     ("ids", (70, 264), "work"), ("off1", (70, 264), "u8")]


def _tile_id(cases):
    return lambda i: f"{i}-{cases[i][0]}-{cases[i][1][0]}x{cases[i][1][1]}-{cases[i][2]}"


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CACHED_TILE_CASES)), ids=_tile_id(CACHED_TILE_CASES))
@pytest.mark.parametrize("pattern,work", INSTANCES)
def test_cached_route_tile_first_pass(ti, dev, pattern, work, i):
    """Route "cached_tile" (EPI_STORE_MINMAX, HOT 1 on IDS frames and HOT 0 on a frame one byte off, then the tails)."""
    way, shape, kind = CACHED_TILE_CASES[i]
    kw, ccm, unit = branches(i)
    odt = work if kind == "work" else kind
    ids = way == "ids"
    what = f"cached_tile {way} {pattern} {work}->{odt} {shape} {kw} ccm {ccm} unit {unit}"
    src = _packed_at(dev, packed_frame(shape, pattern, unit, ids), 0 if ids else 1)
    out = _view_at(dev, shape + (3,), odt, 0)
    image = None if odt == work else _view_at(dev, shape + (3,), work, 0)
    got = run_chain(ti, dev, src, out, image, shape, pattern, ids, work, odt, ccm, kw, "cached_tile", want_hot=1 if ids else 0)
    assert_close(got, reference(shape, pattern, work, odt, i, ids), what)


# (way, shape, output).  "ids" / "off1": the C entry point with a NULL work image on an IDS frame / a frame one byte off;
# "ragged": the Python entry point with W % 8 != 0; "outview": the Python entry point with out= a work-dtype view one
# element off its 16-byte boundary (2 bytes for f16)
RECOMPUTE_CASES = [("ids", (32, 128), "u8"), ("ids", (70, 264), "u16"), ("off1", (34, 136), "u16"), ("off1", (70, 264), "u8"),
                   ("ragged", (34, 130), "work"), ("ragged", (70, 266), "u8"), ("ragged", (34, 130), "u16"),
                   ("ragged", (70, 266), "work"), ("outview", (34, 136), "work"), ("outview", (32, 128), "work")]


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(RECOMPUTE_CASES)), ids=_tile_id(RECOMPUTE_CASES))
@pytest.mark.parametrize("pattern,work", INSTANCES)
def test_recompute_route(ti, dev, pattern, work, i):
    """Route "recompute" (four tile passes and three finalize launches), reached the four ways RECOMPUTE_CASES names."""
    import torch
    from taichi_image_amd import _native
    from taichi_image_amd.pipeline import pipeline12_reinhard
    way, shape, kind = RECOMPUTE_CASES[i]
    kw, ccm, unit = branches(i)
    odt = work if kind == "work" else kind
    ids = way == "ids"
    H, W = shape
    what = f"recompute {way} {pattern} {work}->{odt} {shape} {kw} ccm {ccm} unit {unit}"
    ref = reference(shape, pattern, work, odt, i, ids)
    if way in ("ids", "off1"):
        src = _packed_at(dev, packed_frame(shape, pattern, unit, ids), 0 if ids else 1)
        out = _view_at(dev, shape + (3,), odt, 0)
        got = run_chain(ti, dev, src, out, None, shape, pattern, ids, work, odt, ccm, kw, "recompute")
        assert_close(got, ref, what)
        return
    src = _packed_at(dev, packed_frame(shape, pattern, unit), 0)
    out = _view_at(dev, shape + (3,), odt, SIZE[odt] if way == "outview" else 0)
    for image in ((None,) if odt == work else (None, A)):         # (whatever aligned work image the wrapper brings along)
        name, r = _native.pipeline12_route(src.data_ptr(), out.data_ptr(), image, H, W, 0, CODE[work], CODE[odt])
        assert name == "recompute" and r.rows_per_wave == 0, f"{what}: route {name}"
    got = []
    for rep in range(2):
        out.zero_()
        res = pipeline12_reinhard(src, pattern=ti.BayerPattern(PATTERNS[pattern]), correct_colors=CCM if ccm else None,
                                  work_dtype=work, dtype=odt, out=out, whole_frame=False, **kw)
        torch.cuda.synchronize()
        assert res is out
        got.append(out.cpu().numpy())
    assert_close(got[0], ref, what)
    assert_exact(got[1], got[0], what + ": second launch")


# ---------------------------------------------------------------------------------------------------------------------
# the S_STORE loaders on the same geometry

LOADER_SHAPES = [(4100, 520), (12290, 16), (16396, 16)]           # 3 pairs in two column bands, 4 pairs, 5 pairs
CAMS = [("Camera16", "f16"), ("Camera32", "f32")]
# stream_kernel's LV: 0 no levels, 1 a uniform black level, 2 per site, 3 a lens shading grid
LEVELS = {"none": (None, None, False), "uniform": (300, None, False), "per_site": (PER_SITE, 3900, False),
          "shading": (None, None, True)}
GRID = make_grid(np.random.default_rng(5), 17, 13, 4)


@functools.lru_cache(maxsize=None)
def loader_frame(shape, pattern, k):
    return packed_frame(shape, pattern, False) if k == 0 else \
        _frozen(pairs_frame(shape[0], shape[1], PATTERNS[pattern], True, seed=k))


@functools.lru_cache(maxsize=8)
def loader_ref(shape, pattern, work, levels, k):
    black, white, shading = LEVELS[levels]
    return _frozen(ref_load(loader_frame(shape, pattern, k), 12, work, PATTERNS[pattern], GRID if shading else None, black, white))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LOADER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("levels", list(LEVELS))
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("cam,work", CAMS)
def test_loaders_at_every_ring_class(ti, dev, cam, work, pattern, levels, shape):
    """stream_kernel<E, PR, PC, S_STORE, LV> beyond two row pairs: load_packed12 with the metering subsample on the way
    (metering stride 8) and without (stride 4), and load_packed12_batch of 10 frames (two launches of 8 and 2), bit for
    bit against ref_load; the tagged subsample is image[::8, ::8] (its rows fall in different rotations of the ring at
    different rows per wave)."""
    import torch
    from taichi_image_amd import _native
    H, W = shape
    black, white, shading = LEVELS[levels]
    what = f"{cam} {pattern} {levels} {shape}"
    assert _native.lib().mi_isp_load_packed_metered_is_fused(H, W, 12, 0, CODE[work], 8) == 1, what
    name, r = _native.pipeline12_route(A, A, None, H, W, 0, CODE[work], CODE[work])
    assert name == "stream" and r.rows_per_wave == 2 * STREAM_CLASS[shape][0], what      # (the loaders share strm::geometry)
    make = lambda stride: getattr(ti, cam)(ti.BayerPattern(PATTERNS[pattern]), device=dev, black_level=black,
                                           white_level=white, lens_shading=GRID if shading else None, metering_stride=stride)
    n_distinct = 2 if W == 16 else 1                            # (the wide frame's reference takes a second: one frame there)
    refs = [loader_ref(shape, pattern, work, levels, k) for k in range(n_distinct)]
    srcs = [torch.from_numpy(np.array(loader_frame(shape, pattern, k))).to(dev) for k in range(n_distinct)]
    metered, plain = make(8), make(4)
    got = metered.load_packed12(srcs[0])
    sub = getattr(got, "_mi_metering_sub", None)
    assert sub is not None and sub[1] == 8, what + ": no subsample on the way"
    assert_exact(got.cpu().numpy(), refs[0], what + ": metered load")
    assert_exact(sub[0].cpu().numpy(), np.ascontiguousarray(refs[0][::8, ::8]), what + ": subsample")
    got = plain.load_packed12(srcs[0])
    assert getattr(got, "_mi_metering_sub", None) is None
    assert_exact(got.cpu().numpy(), refs[0], what + ": plain load")
    batch = metered.load_packed12_batch([srcs[k % n_distinct] for k in range(10)])
    assert len(batch) == 10
    for k, g in enumerate(batch):
        ref = refs[k % n_distinct]
        assert_exact(g.cpu().numpy(), ref, what + f": batch frame {k}")
        sub = getattr(g, "_mi_metering_sub", None)
        assert sub is not None and sub[1] == 8
        assert_exact(sub[0].cpu().numpy(), np.ascontiguousarray(ref[::8, ::8]), what + f": batch frame {k} subsample")
