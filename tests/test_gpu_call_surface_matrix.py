"""The kernels behind the standalone call surface (csrc/isp_elementwise.hip), instance by instance against
oracle/isp_oracle.py on seeded inputs:

  packed.decode12 / decode16 / encode12     decode12_kernel<T>, decode16_kernel<T>, encode12_kernel<T>
  mi_isp_load_convert (C ABI)               load_convert_kernel<T>, 3 modes
  bayer.rgb_to_bayer                        mosaic_kernel<T>
  interpolate.resize_bilinear / transform   resize_kernel<TI, TO>, transform_kernel<T>
  color.rgb_yuv420_image / yuv420_rgb_image rgb_yuv420_vec_kernel / rgb_yuv420_kernel<TI, TO>, yuv420_rgb_kernel<TI, TO>
  tonemap.tonemap_linear / tonemap_reinhard rgb_pass_kernel<TI, TO, PM_MINMAX / PM_STATS / PM_RH_MINMAX / PM_RH_STORE /
                                            PM_LINEAR_STORE>

Every (TI, TO) pair - every dtype where a kernel has one - meets the oracle at least once, at the project's contract:
assert_exact for unpack, encode, mosaic, transform, load_convert and resize, assert_close with its defaults for the
tonemaps and the YUV conversions.  Case ids read in-out-shape class-route.

Routes come from the library: mi_isp_rgb_to_yuv420_is_vector says which YUV kernel the ACTUAL pointers of a call get,
mi_isp_tonemap_pass_geometry the grids and the FULL / general split of a tonemap's passes; both are the functions the
launches read.  The tonemap shape classes (asserted from the query, TM_CLASS):

  A  (1, 3)        one ragged group, no FULL group
  B  (16, 64)      1024 px: exactly two whole waves, no general group
  C  (50, 70)      3500 px: 384 FULL groups, 53 whole general groups, a 4-pixel tail; runs all 16 pairs
  D  (66, 94)      two blocks: the fold of the next pass reads two partial results
  E  (1031, 2052)  2,115,612 px: the 512-block store passes take a second grid-stride step, the 256-block reduce passes a
                   third; three whole general groups and a 4-pixel tail behind the FULL groups

Classes B and C also run through the C ABI on views one element off their alignment (source, destination, both): no FULL
group is left, and every result is the aligned call's bit for bit; class E once with both buffers off, where the general
loop - which aligned buffers leave at most 63 groups and a tail - strides the grids itself.  The scenes are lifted off
black, so a zero taken in from beyond a ragged tail moves the bounds.

Three constants carry the "wrap" shapes (every kernel launched with grid_for, and both pass grids, once beyond the first
sweep of its grid): GRID_FOR_LANES, STORE_SWEEP_PX, REDUCE_SWEEP_PX below, each with the line it restates.

The first tests need no GPU: the tables hold what they claim, the wrap shapes exceed their constants, the shape classes
have the group arithmetic claimed (read from the query), the YUV route query gives the expected route for every shape
of the tables, and - on the oracle alone - every wrap case's reference differs between the first sweep and the rest.

Not here: metering; the ISP's batched passes (PM_ISP_*), the whole-frame, camera-group and multi-pass kernels (their own
files)."""
import functools

import numpy as np
import pytest

from oracle import isp_oracle as O
from tests.util import assert_close, assert_exact, natural_packed12

DT = ["u8", "u16", "f16", "f32"]
PAIRS = [(a, b) for a in DT for b in DT]
FOUR = [("u8", "f32"), ("u16", "f16"), ("f16", "u16"), ("f32", "u8")]      # every TI and every TO once
CODE = {"u8": 0, "u16": 1, "f16": 2, "f32": 3}                              # MI_U8 .. MI_F32
SIZE = {"u8": 1, "u16": 2, "f16": 2, "f32": 4}
NP = O.NP_DTYPE

# csrc/isp_elementwise.hip, grid_for(): `int cap = 256 * 16` blocks of EW_THREADS = 256 lanes
GRID_FOR_LANES = 256 * 16 * 256
# csrc/isp_elementwise.hip, pass_blocks(): `reduce_only ? 256 : 512` blocks of PASS_THREADS = 512 lanes, one 8-pixel group
# per lane and step
STORE_SWEEP_PX = 512 * 512 * 8
REDUCE_SWEEP_PX = 256 * 512 * 8
assert GRID_FOR_LANES == 1_048_576

A = 0x7F0000000000                                                          # made-up addresses: the queries never dereference


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _rng(*key):
    return np.random.default_rng([20260, *[int(k) for k in key]])


def _random(rng, shape, dt, lo=0.0, hi=1.0):
    """Full-range integers, or floats of [lo, hi)."""
    if dt in ("u8", "u16"):
        return rng.integers(0, int(O.SCALE[dt]) + 1, shape).astype(NP[dt])
    return (rng.random(shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).astype(NP[dt])


def wrap_is_informative(items, sweep, what):
    """items: the reference, one row per work item in the kernel's item order.  The rows beyond the first sweep of the
    grid are neither constant nor a repeat of the rows the same lanes wrote in the first sweep."""
    items = np.asarray(items)
    items = items.reshape(items.shape[0], -1)
    tail = items[sweep:]
    assert tail.shape[0] > 0, f"{what}: {items.shape[0]} items do not leave the first sweep of {sweep}"
    assert np.unique(tail).size > 1, f"{what}: constant beyond the first sweep"
    assert not np.array_equal(tail, items[:tail.shape[0]]), f"{what}: the second sweep repeats the first"
    assert np.unique(items[:sweep]).size > 1, f"{what}: constant first sweep"


# ---------------------------------------------------------------------------------------------------------------------
# stateless tonemaps

TM_OPS = {"linear": None, "reinhard_ca0": 0.0, "reinhard_ca03": 0.3}        # color_adapt: the CA0 and the three-pow variant
TM_GAMMA, TM_INTENSITY, TM_LIGHT = 0.6, 1.2, 0.8
# shape -> (class, blocks of a storing pass, blocks of a reduce pass, FULL groups, whole general groups, tail pixels)
TM_CLASS = {(1, 3): ("A", 1, 1, 0, 0, 3), (16, 64): ("B", 1, 1, 128, 0, 0), (50, 70): ("C", 1, 1, 384, 53, 4),
            (66, 94): ("D", 2, 2, 768, 7, 4), (1031, 2052): ("E", 512, 256, 264448, 3, 4)}
TM_CASES = [(p, (50, 70)) for p in PAIRS] + [(p, s) for s in ((1, 3), (16, 64), (66, 94)) for p in FOUR] + \
           [(p, (1031, 2052)) for p in (("f16", "u8"), ("u16", "u16"))]
TM_ALIGN_PAIRS = [("f16", "u8"), ("u8", "u8"), ("u16", "u16"), ("f32", "f32")]
TM_ALIGN_SHAPES = [(16, 64), (50, 70)]


def tm_geometry_of(shape):
    """What mi_isp_tonemap_pass_geometry must give for aligned buffers of a class."""
    _, nb, nbr, full, whole, tail = TM_CLASS[shape]
    return (nb, nbr, full, whole + (1 if tail else 0))


@functools.lru_cache(maxsize=None)
def tm_scene(shape):
    """natural_packed12 -> bayer_to_rgb as in tests/test_gpu_parity.py, f32; an odd size is cut from the next even one.
    The scene is lifted off black (dark=-0.15): its minimum stays well above 0, so a zero that a reduction takes in from
    beyond a ragged tail moves the bounds (test_tonemap_scenes_are_off_black; added for the mutation that lets PM_MINMAX
    read one pixel beyond the tail, which a scene with black pixels showed in class A only)."""
    H, W = shape
    He, We = H + H % 2, W + W % 2
    rgb = O.bayer_to_rgb(O.decode12(natural_packed12(_rng(1, H, W), He, We, dark=-0.15), "f32", scaled=True))
    return _frozen(rgb[:H, :W])


@functools.lru_cache(maxsize=None)
def tm_image(shape, din):
    x = tm_scene(shape)
    if din in ("u8", "u16"):
        return _frozen((x * np.float32(O.SCALE[din])).astype(NP[din]))      # the full integer range
    return _frozen(x.astype(NP[din]))


@functools.lru_cache(maxsize=None)
def tm_ref(op, shape, din, dout):
    img = tm_image(shape, din)
    if op == "linear":
        return _frozen(O.tonemap_linear(img, TM_GAMMA, dout))
    return _frozen(O.tonemap_reinhard(img, TM_GAMMA, TM_INTENSITY, TM_LIGHT, TM_OPS[op], dout))


def tm_id(case):
    (din, dout), shape = case
    cls, nb, _, full, whole, tail = TM_CLASS[shape]
    route = "general" if full == 0 else ("full" if whole + tail == 0 else "full+general")
    if nb == 512:
        route += "+wrap"
    return f"{din}-{dout}-{cls}_{shape[0]}x{shape[1]}-{route}"


# ---------------------------------------------------------------------------------------------------------------------
# YUV 4:2:0

YUV_FWD_SHAPES = [(8, 32), (6, 10), (6, 16)]
# the route by output dtype: at (6, 16) a chroma plane has 24 elements - 24 bytes of u8 are no multiple of 16, 48 and 96 are
YUV_ROUTE = {(8, 32): dict(u8="vector", u16="vector", f16="vector", f32="vector"),
             (6, 10): dict(u8="scalar", u16="scalar", f16="scalar", f32="scalar"),
             (6, 16): dict(u8="scalar", u16="vector", f16="vector", f32="vector"),
             (2056, 2056): dict(u8="scalar"), (2056, 8192): dict(u8="vector")}
YUV_INV_SHAPES = [(12, 16), (66, 70)]
YUV_WRAP_INV = ((1032, 1024), "u16", "u8")
YUV_WRAP_SCALAR = ((2056, 2056), "u8", "u8")
YUV_WRAP_VECTOR = ((2056, 8192), "u8", "u8")


@functools.lru_cache(maxsize=None)
def yuv_rgb_in(shape, din):
    """Floats reach slightly outside [0, 1] (a negative float -> unsigned cast saturates to 0 in oracle and library)."""
    return _frozen(_random(_rng(2, *shape, CODE[din]), shape + (3,), din, -0.05, 1.15))


@functools.lru_cache(maxsize=None)
def yuv_fwd_ref(shape, din, dout):
    return _frozen(O.rgb_yuv420(yuv_rgb_in(shape, din), dout))


@functools.lru_cache(maxsize=None)
def yuv_planes_in(shape, din, pushed):
    """The oracle's forward output of a random image, converted to TI; pushed: chroma moved towards 0 and 1, so that the
    RGB result leaves [0, 1] on both sides."""
    H, W = shape
    yuv = np.array(O.rgb_yuv420(_random(_rng(3, H, W), shape + (3,), "f32"), "f32"))
    if pushed:
        c = yuv[H:]
        yuv[H:] = np.where(c > 0.5, 1.0 - (1.0 - c) * 0.1, c * 0.1)
    yuv = np.clip(yuv, 0.0, 1.0)
    if din in ("u8", "u16"):
        return _frozen((yuv * np.float32(O.SCALE[din])).astype(NP[din]))
    return _frozen(yuv.astype(NP[din]))


@functools.lru_cache(maxsize=None)
def yuv_inv_ref(shape, din, dout, pushed):
    return _frozen(O.yuv420_rgb(yuv_planes_in(shape, din, pushed), dout))


# ---------------------------------------------------------------------------------------------------------------------
# resize, transform, mosaic

RESIZE_SRC = (61, 83)
RESIZE_WRAP = ((600, 640), 1.7, "u8", "u16")


def resize_size(src_shape, scale, extra=0):
    """(w, h) of int(scale * src) per axis, as the call surface's scale_bilinear; extra: pixels beyond it on both axes."""
    s = scale if isinstance(scale, tuple) else (scale, scale)
    return (int(src_shape[1] * s[1]) + extra, int(src_shape[0] * s[0]) + extra)


# (pair, scale, extra)
RESIZE_CASES = [(p, s, 0) for s in (0.8, 1.7) for p in PAIRS] + [(p, (0.3515625, 0.46875), 0) for p in FOUR] + \
               [(p, 1.7, 2) for p in FOUR]


def resize_id(case):
    (din, dout), scale, extra = case
    s = "x".join(str(v) for v in scale) if isinstance(scale, tuple) else str(scale)
    return f"{din}-{dout}-{RESIZE_SRC[0]}x{RESIZE_SRC[1]}_s{s}-{'edge+2' if extra else 'grid'}"


@functools.lru_cache(maxsize=None)
def resize_src(shape, din):
    return _frozen(_random(_rng(4, *shape, CODE[din]), shape + (3,), din))


@functools.lru_cache(maxsize=None)
def resize_ref(shape, din, dout, scale, extra):
    return _frozen(O.resize_bilinear(resize_src(shape, din), resize_size(shape, scale, extra), scale, dout))


TRANSFORM_SHAPE, TRANSVERSE_SHAPE = (34, 130), (34, 34)
TRANSFORM_WRAP = [("u16", "rotate_90"), ("f32", "flip_horiz")]
MOSAIC_SHAPE = (34, 36)
WRAP_IMAGE = (1032, 1024)                                                   # transform, mosaic and the inverse YUV


@functools.lru_cache(maxsize=None)
def image_of(shape, dt):
    return _frozen(_random(_rng(5, *shape, CODE[dt]), shape + (3,), dt))


# ---------------------------------------------------------------------------------------------------------------------
# packed, load_convert

D12_PAIRS = 4 * 300 + 3                                                     # fast groups of 4 pairs plus a scalar tail
D16_N = 8 * 300 + 5
E12_PAIRS = 4 * 300 + 3
D12_WRAP = ("f16", True, False, 4 * GRID_FOR_LANES + 4 * 300 + 3)           # dtype, scaled, ids, pairs (fast path)
D12_WRAP_BYTES = ("u16", False, True, GRID_FOR_LANES + 300)                 # a view one byte in: one pair per lane
D16_WRAP = ("u8", True, 8 * GRID_FOR_LANES + 8 * 300 + 5)
E12_WRAP = ("u16", True, False, GRID_FOR_LANES + 300)
LC_N = 256 * 5 + 3
LC_MODES = {"16u": (0, O.load_16u), "32f": (1, O.load_32f), "16f": (2, O.load_16f)}      # MI_LOAD_16U / 32F / 16F
LC_WRAP = ("16u", "f16", GRID_FOR_LANES + 300)
PACKED_CASES = [(dt, scaled, ids) for dt in DT for scaled in (False, True) for ids in (False, True)]


@functools.lru_cache(maxsize=None)
def packed_bytes(n, seed):
    return _frozen(_rng(6, seed, n).integers(0, 256, n).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def encode_values(n, dt, scaled):
    """Unscaled floats hold integers of [0, 4095]; scaled inputs reach below 0 and above the type's scale - and far enough
    above it for the clamp to 65535."""
    rng = _rng(7, n, CODE[dt], scaled)
    if dt in ("u8", "u16"):
        return _frozen(_random(rng, n, dt))
    if not scaled:
        return _frozen(rng.integers(0, 4096, n).astype(NP[dt]))
    v = _random(rng, n, dt, -0.2, 1.2)
    v[5::97] = 20.0
    v[11::89] = -3.0
    return _frozen(v)


@functools.lru_cache(maxsize=None)
def lc_src(mode, n):
    rng = _rng(8, n)
    if mode == "32f":
        return _frozen(_random(rng, n, "f32", -0.5, 1.5))
    return _frozen(rng.integers(0, 65536, n).astype(np.uint16))


# ---------------------------------------------------------------------------------------------------------------------
# premises (no GPU)

def test_tables_hold_what_they_claim():
    assert len(PAIRS) == 16 and len(set(PAIRS)) == 16 and {p[0] for p in PAIRS} == {p[1] for p in PAIRS} == set(DT)
    assert {p[0] for p in FOUR} == {p[1] for p in FOUR} == set(DT)
    assert {p for p, s in TM_CASES if s == (50, 70)} == set(PAIRS)
    for shape in ((1, 3), (16, 64), (66, 94)):
        mine = [p for p, s in TM_CASES if s == shape]
        assert {p[0] for p in mine} == {p[1] for p in mine} == set(DT), shape
    assert [p for p, s in TM_CASES if s == (1031, 2052)] == [("f16", "u8"), ("u16", "u16")]
    assert {s for _, s in TM_CASES} == set(TM_CLASS) and sorted(c[0] for c in TM_CLASS.values()) == list("ABCDE")
    assert set(TM_OPS) == {"linear", "reinhard_ca0", "reinhard_ca03"} and TM_OPS["reinhard_ca0"] == 0.0 != TM_OPS["reinhard_ca03"]
    assert TM_GAMMA != 1.0                                                   # the pow of the final pass runs
    for scale in (0.8, 1.7):
        assert {c[0] for c in RESIZE_CASES if c[1] == scale and c[2] == 0} == set(PAIRS)
    assert {c[0] for c in RESIZE_CASES if isinstance(c[1], tuple)} == set(FOUR)
    assert {c[0] for c in RESIZE_CASES if c[2] == 2} == set(FOUR)
    assert len(PACKED_CASES) == 16 and {c[0] for c in PACKED_CASES} == set(DT)
    assert len(O.TRANSFORMS) == 8 and set(LC_MODES) == {"16u", "32f", "16f"}
    for shape, by_out in YUV_ROUTE.items():
        assert set(by_out) <= set(DT) and (shape[0] > 2000 or set(by_out) == set(DT))
    assert set(YUV_FWD_SHAPES) | {YUV_WRAP_SCALAR[0], YUV_WRAP_VECTOR[0]} == set(YUV_ROUTE)


def test_wrap_shapes_exceed_their_sweeps():
    H, W = 1031, 2052
    assert H * W > STORE_SWEEP_PX and H * W > 2 * REDUCE_SWEEP_PX           # a second step; a third
    (H, W), _, _ = YUV_WRAP_INV
    assert H * W > GRID_FOR_LANES                                           # yuv420_rgb_kernel: one lane per pixel
    (H, W), _, _ = YUV_WRAP_SCALAR
    assert W % 16 == 8 and (H // 2) * (W // 2) == 1_056_784 > GRID_FOR_LANES          # one lane per 2 x 2 block
    (H, W), _, _ = YUV_WRAP_VECTOR
    assert W % 16 == 0 and (H // 2) * (W // 8) == 1_052_672 > GRID_FOR_LANES          # one lane per 2 rows x 8 pixels
    src, scale, _, _ = RESIZE_WRAP
    w, h = resize_size(src, scale)
    assert (h, w) == (1020, 1088) and h * w == 1_109_760 > GRID_FOR_LANES
    assert WRAP_IMAGE[0] * WRAP_IMAGE[1] > GRID_FOR_LANES and WRAP_IMAGE[0] % 2 == 0 and WRAP_IMAGE[0] != WRAP_IMAGE[1]
    assert D12_WRAP[3] // 4 > GRID_FOR_LANES and D12_WRAP[3] % 4 == 3       # fast groups beyond the sweep, then a tail
    assert D12_WRAP_BYTES[3] > GRID_FOR_LANES
    assert D16_WRAP[2] // 8 > GRID_FOR_LANES and D16_WRAP[2] % 8 == 5
    assert E12_WRAP[3] > GRID_FOR_LANES and LC_WRAP[2] > GRID_FOR_LANES
    assert D12_PAIRS % 4 == 3 and D12_PAIRS // 4 > 256 and D16_N % 8 == 5 and D16_N // 8 > 256 and LC_N > 4 * 256


def test_tonemap_classes_have_the_group_arithmetic_claimed():
    """From mi_isp_tonemap_pass_geometry on made-up aligned addresses: if pass_blocks or the FULL rule changes, these are
    the shapes to move.  A view one element off has no FULL group at all."""
    from taichi_image_amd import _native
    for shape, (cls, nb, nbr, full, whole, tail) in TM_CLASS.items():
        H, W = shape
        n_px = H * W
        assert tail == n_px % 8 and full + whole == n_px // 8, shape
        for din, dout in PAIRS:
            what = f"class {cls} {shape} {din}->{dout}"
            assert _native.tonemap_pass_geometry(H, W, CODE[din], CODE[dout], A, A + (1 << 32)) == tm_geometry_of(shape), what
            groups = -(-n_px // 8)
            for s_off, d_off in ((SIZE[din], 0), (0, SIZE[dout]), (SIZE[din], SIZE[dout])):
                geo = _native.tonemap_pass_geometry(H, W, CODE[din], CODE[dout], A + s_off, A + (1 << 32) + d_off)
                assert geo == (nb, nbr, 0, groups), f"{what} +{s_off} +{d_off}: {geo}"
    cls = {c[0]: c for c in TM_CLASS.values()}
    assert cls["A"][3:] == (0, 0, 3)                                         # one ragged group
    assert cls["B"][3:] == (128, 0, 0) and cls["B"][3] % 64 == 0             # two whole waves and nothing else
    assert cls["C"][3:] == (384, 53, 4)
    assert cls["D"][1:3] == (2, 2)
    assert cls["E"][1:3] == (512, 256) and cls["E"][4:] == (3, 4)
    L = _native.lib()
    out = (_native.c_int64 * 4)()
    assert L.mi_isp_tonemap_pass_geometry(0, 4, 0, 0, A, A, out) != 0 and b"shape" in L.mi_isp_last_error()
    assert L.mi_isp_tonemap_pass_geometry(4, 4, 0, 0, None, A, out) != 0 and b"null" in L.mi_isp_last_error()
    assert L.mi_isp_tonemap_pass_geometry(4, 4, 0, 9, A, A, out) != 0


def test_tonemap_scenes_are_off_black():
    """Every tonemap input has a minimum well above 0 and a range to normalise, in every input dtype: a lane that takes
    in the zero padding behind a ragged tail, or a fold that reads a partial result nobody wrote, moves the bounds."""
    for shape in TM_CLASS:
        for din in DT:
            x = tm_image(shape, din).astype(np.float64) / O.SCALE[din]
            assert x.min() > 0.05 and x.max() - x.min() > 0.3, f"{shape} {din}: {x.min()} .. {x.max()}"


def test_yuv_route_query_gives_the_expected_route():
    """mi_isp_rgb_to_yuv420_is_vector on made-up addresses: every shape of the tables at every output dtype - the flip at
    (6, 16) with the output dtype alone - and either pointer 4 or 8 bytes off."""
    from taichi_image_amd import _native
    for shape, by_out in YUV_ROUTE.items():
        H, W = shape
        for dout, want in by_out.items():
            got = _native.rgb_to_yuv420_is_vector(A, A + (1 << 32), H, W, CODE[dout])
            assert got == (want == "vector"), f"{shape} -> {dout}: vector {got}, the table says {want}"
            for r_off, y_off in ((4, 0), (0, 4), (0, 8), (8, 8)):
                assert not _native.rgb_to_yuv420_is_vector(A + r_off, A + (1 << 32) + y_off, H, W, CODE[dout]), (shape, dout)
    assert YUV_ROUTE[(6, 16)] == dict(u8="scalar", u16="vector", f16="vector", f32="vector")
    assert (6 // 2) * (16 // 2) == 24                                        # elements of a chroma plane
    L = _native.lib()
    assert L.mi_isp_rgb_to_yuv420_is_vector(None, A, 8, 32, 0) < 0 and b"null" in L.mi_isp_last_error()
    assert L.mi_isp_rgb_to_yuv420_is_vector(A, A, 7, 32, 0) < 0 and b"even" in L.mi_isp_last_error()
    assert L.mi_isp_rgb_to_yuv420_is_vector(A, A, 8, 32, 7) < 0


def test_wrap_references_differ_beyond_the_first_sweep():
    """On the oracle alone: constant data beyond the first sweep would prove nothing."""
    for op in TM_OPS:
        for din, dout in (("f16", "u8"), ("u16", "u16")):
            ref = tm_ref(op, (1031, 2052), din, dout)
            full = TM_CLASS[(1031, 2052)][3]
            wrap_is_informative(ref.reshape(-1)[:full * 24].reshape(-1, 24), STORE_SWEEP_PX // 8, f"tonemap {op} {din}->{dout}")
    (H, W), din, dout = YUV_WRAP_INV
    wrap_is_informative(yuv_inv_ref((H, W), din, dout, False).reshape(-1, 3), GRID_FOR_LANES, "yuv420_rgb")
    (H, W), din, dout = YUV_WRAP_SCALAR
    wrap_is_informative(yuv_fwd_ref((H, W), din, dout)[H:].reshape(2, -1)[1].reshape(-1, 1), GRID_FOR_LANES, "rgb_yuv420 scalar")
    (H, W), din, dout = YUV_WRAP_VECTOR
    wrap_is_informative(yuv_fwd_ref((H, W), din, dout)[H:].reshape(2, -1)[1].reshape(-1, 4), GRID_FOR_LANES, "rgb_yuv420 vector")
    src, scale, din, dout = RESIZE_WRAP
    wrap_is_informative(resize_ref(src, din, dout, scale, 0).reshape(-1, 3), GRID_FOR_LANES, "resize")
    for dt, name in TRANSFORM_WRAP:
        wrap_is_informative(O.transform(image_of(WRAP_IMAGE, dt), name).reshape(-1, 3), GRID_FOR_LANES, f"transform {name}")
    wrap_is_informative(O.rgb_to_bayer(image_of(WRAP_IMAGE, "u16"), 1).reshape(-1, 1), GRID_FOR_LANES, "rgb_to_bayer")
    dt, scaled, ids, pairs = D12_WRAP
    ref = O.decode12(packed_bytes(pairs * 3, 12), dt, scaled, ids)
    wrap_is_informative(ref[:pairs // 4 * 8].reshape(-1, 8), GRID_FOR_LANES, "decode12")
    dt, scaled, ids, pairs = D12_WRAP_BYTES
    wrap_is_informative(O.decode12(packed_bytes(pairs * 3 + 1, 13)[1:], dt, scaled, ids).reshape(-1, 2), GRID_FOR_LANES, "decode12 bytes")
    dt, scaled, n = D16_WRAP
    wrap_is_informative(O.decode16(packed_bytes(n * 2, 16), dt, scaled)[:n // 8 * 8].reshape(-1, 8), GRID_FOR_LANES, "decode16")
    dt, scaled, ids, pairs = E12_WRAP
    wrap_is_informative(O.encode12(encode_values(2 * pairs, dt, scaled), scaled, ids).reshape(-1, 3), GRID_FOR_LANES, "encode12")
    mode, dout, n = LC_WRAP
    wrap_is_informative(LC_MODES[mode][1](lc_src(mode, n), dout).reshape(-1, 1), GRID_FOR_LANES, "load_convert")


def test_pushed_chroma_leaves_the_unit_range():
    """The inverse YUV cases' second input: the reference clamps from above only, so float results keep negatives and
    unsigned ones saturate at 0 - and both sides are reached."""
    for shape in YUV_INV_SHAPES:
        f = yuv_inv_ref(shape, "f32", "f32", True)
        assert f.min() < -0.05 and f.max() == 1.0 and (f == 1.0).mean() > 0.01, shape
        u = yuv_inv_ref(shape, "f32", "u8", True)
        assert (u[f < 0] == 0).all() and (u == 255).any() and (u == 0).any(), shape


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


def tok(ti, name):
    return getattr(ti.types, name)


def _torch_dtype(name):
    import torch
    return {"u8": torch.uint8, "u16": torch.uint16, "f16": torch.float16, "f32": torch.float32}[name]


def _up(dev, a):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)


def _view_at(dev, shape, dtype_name, offset, fill=None):
    """A contiguous tensor of that shape and dtype whose first byte lies `offset` bytes into a fresh (aligned) buffer,
    with 8 KiB of the buffer behind it (a wave's 64 groups of f32 are 6 KiB: a store that a mutant of the FULL path
    misplaces within its wave still lands in this storage)."""
    import torch
    n = int(np.prod(shape)) * SIZE[dtype_name]
    buf = torch.zeros(n + 8192, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    t = buf[offset:offset + n].view(_torch_dtype(dtype_name)).view(*shape)
    assert t.data_ptr() == buf.data_ptr() + offset and t.is_contiguous()
    if fill is not None:
        t.copy_(_up(dev, fill))
    return t


def _tonemap(ti, op, src, dout):
    if op == "linear":
        return ti.tonemap.tonemap_linear(src, gamma=TM_GAMMA, dtype=tok(ti, dout))
    return ti.tonemap.tonemap_reinhard(src, gamma=TM_GAMMA, intensity=TM_INTENSITY, light_adapt=TM_LIGHT,
                                       color_adapt=TM_OPS[op], dtype=tok(ti, dout))


@pytest.mark.gpu
@pytest.mark.parametrize("case", TM_CASES, ids=tm_id)
@pytest.mark.parametrize("op", list(TM_OPS))
def test_tonemap_instances_at_every_class(ti, dev, op, case):
    """tonemap_linear (PM_MINMAX, PM_LINEAR_STORE) and tonemap_reinhard (PM_MINMAX, PM_STATS, PM_RH_MINMAX, PM_RH_STORE),
    color_adapt 0 and 0.3, through the call surface; the class is asserted from the query on the call's own pointers."""
    from taichi_image_amd import _native
    (din, dout), shape = case
    H, W = shape
    src = _up(dev, tm_image(shape, din))
    got = _tonemap(ti, op, src, dout)
    geo = _native.tonemap_pass_geometry(H, W, CODE[din], CODE[dout], src.data_ptr(), got.data_ptr())
    assert geo == tm_geometry_of(shape), f"geometry {geo}, class {TM_CLASS[shape][0]} was written for {tm_geometry_of(shape)}"
    assert_close(got.cpu().numpy(), tm_ref(op, shape, din, dout), f"{op} {tm_id(case)}")


def _tonemap_abi(dev, op, src, out, H, W, din, dout):
    import torch
    from taichi_image_amd import _native
    L, ws = _native.lib(), _native.workspace(H, W, dev)
    if op == "linear":
        _native.check(L.mi_isp_tonemap_linear(src.data_ptr(), out.data_ptr(), H, W, CODE[din], CODE[dout], TM_GAMMA,
                                              ws.data_ptr(), _native.stream_ptr(dev)))
    else:
        _native.check(L.mi_isp_tonemap_reinhard(src.data_ptr(), out.data_ptr(), H, W, CODE[din], CODE[dout], TM_GAMMA,
                                                TM_INTENSITY, TM_LIGHT, TM_OPS[op], ws.data_ptr(), _native.stream_ptr(dev)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TM_ALIGN_SHAPES, ids=lambda s: f"{TM_CLASS[s][0]}_{s[0]}x{s[1]}-unaligned")
@pytest.mark.parametrize("din,dout", TM_ALIGN_PAIRS)
@pytest.mark.parametrize("op", list(TM_OPS))
def test_tonemap_unaligned_views(ti, dev, op, din, dout, shape):
    """Through the C ABI: the source one element into its storage (vec_in == 0), the destination (vec_out == 0: aligned
    loads, scalar stores, every whole group demoted from the FULL path - in class B all 128 run the general path with
    npx == 8), both.  Same arithmetic, different IO: the bits of the aligned call, and the oracle."""
    from taichi_image_amd import _native
    H, W = shape
    groups = -(-H * W // 8)
    ref = tm_ref(op, shape, din, dout)
    results = {}
    for s_off, d_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
        src = _view_at(dev, shape + (3,), din, s_off * SIZE[din], tm_image(shape, din))
        out = _view_at(dev, shape + (3,), dout, d_off * SIZE[dout])
        geo = _native.tonemap_pass_geometry(H, W, CODE[din], CODE[dout], src.data_ptr(), out.data_ptr())
        want = tm_geometry_of(shape) if (s_off, d_off) == (0, 0) else tm_geometry_of(shape)[:2] + (0, groups)
        assert geo == want, f"src +{s_off} dst +{d_off}: geometry {geo}, expected {want}"
        results[(s_off, d_off)] = _tonemap_abi(dev, op, src, out, H, W, din, dout)
        assert_close(results[(s_off, d_off)], ref, f"{op} {din}->{dout} {shape} src +{s_off} dst +{d_off}")
    for key in ((1, 0), (0, 1), (1, 1)):
        assert_exact(results[key], results[(0, 0)], f"{op} {din}->{dout} {shape} src +{key[0]} dst +{key[1]} against the aligned call")


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["linear", "reinhard_ca03"])
def test_tonemap_unaligned_view_beyond_the_first_sweep(ti, dev, op):
    """Class E, f16 -> u8, both buffers one element off: all 264,452 groups run the general loop, which then strides the
    512-block grid of the storing passes twice and the 256-block grid of the reduce passes three times (with aligned
    buffers it never takes a second step: at most 63 whole groups and a tail are left to it).  Added for the mutation
    that doubles the general loop's stride."""
    from taichi_image_amd import _native
    shape, din, dout = (1031, 2052), "f16", "u8"
    H, W = shape
    src = _view_at(dev, shape + (3,), din, SIZE[din], tm_image(shape, din))
    out = _view_at(dev, shape + (3,), dout, SIZE[dout])
    geo = _native.tonemap_pass_geometry(H, W, CODE[din], CODE[dout], src.data_ptr(), out.data_ptr())
    assert geo == (512, 256, 0, -(-H * W // 8)) and geo[3] * 8 > STORE_SWEEP_PX, geo
    assert_close(_tonemap_abi(dev, op, src, out, H, W, din, dout), tm_ref(op, shape, din, dout), f"{op} f16-u8-E-general-wrap")


def _yuv_in(dev, shape, din):
    return _up(dev, yuv_rgb_in(shape, din))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", YUV_FWD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("din,dout", PAIRS)
def test_rgb_yuv420_instances_and_routes(ti, dev, din, dout, shape):
    """All 16 pairs on the vector kernel (8, 32), on the scalar kernel (6, 10) and at (6, 16), where the plane-size term
    alone decides: scalar for u8 out, vector for the rest.  The route is asked of the call's own pointers."""
    from taichi_image_amd import _native, color
    H, W = shape
    src = _yuv_in(dev, shape, din)
    got = color.rgb_yuv420_image(src, dtype=dout)
    route = "vector" if _native.rgb_to_yuv420_is_vector(src.data_ptr(), got.data_ptr(), H, W, CODE[dout]) else "scalar"
    assert route == YUV_ROUTE[shape][dout], f"{din}->{dout} {shape}: {route}, the case was written for {YUV_ROUTE[shape][dout]}"
    assert_close(got.cpu().numpy(), yuv_fwd_ref(shape, din, dout), f"rgb_yuv420 {din}-{dout}-{H}x{W}-{route}")


@pytest.mark.gpu
@pytest.mark.parametrize("din,dout", PAIRS, ids=lambda v: v)
def test_rgb_yuv420_scalar_by_pointer_alone(ti, dev, din, dout):
    """(8, 32) through the C ABI with yuv 4 bytes into its storage: the scalar kernel for the pointer's sake only, and the
    bits of the vector kernel on the aligned buffer."""
    import torch
    from taichi_image_amd import _native
    shape = (8, 32)
    H, W = shape
    src = _view_at(dev, shape + (3,), din, 0, yuv_rgb_in(shape, din))
    got = {}
    for off, want in ((0, True), (4, False)):
        yuv = _view_at(dev, (H * 3 // 2, W), dout, off)
        assert _native.rgb_to_yuv420_is_vector(src.data_ptr(), yuv.data_ptr(), H, W, CODE[dout]) is want, f"yuv +{off}"
        _native.check(_native.lib().mi_isp_rgb_to_yuv420(src.data_ptr(), yuv.data_ptr(), H, W, CODE[din], CODE[dout],
                                                         _native.stream_ptr(dev)))
        torch.cuda.synchronize()
        got[off] = yuv.cpu().numpy()
        assert_close(got[off], yuv_fwd_ref(shape, din, dout), f"rgb_yuv420 {din}-{dout}-8x32-yuv+{off}")
    assert_exact(got[4], got[0], f"rgb_yuv420 {din}-{dout}: scalar against vector kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", YUV_INV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-grid")
@pytest.mark.parametrize("din,dout", PAIRS)
def test_yuv420_rgb_instances(ti, dev, din, dout, shape):
    """All 16 pairs on the oracle's forward output, and on one with the chroma pushed towards 0 and 1: the reference clamps
    from above only, so float outputs keep negatives and unsigned outputs saturate at 0."""
    from taichi_image_amd import color
    for pushed in (False, True):
        got = color.yuv420_rgb_image(_up(dev, yuv_planes_in(shape, din, pushed)), dtype=dout)
        assert_close(got.cpu().numpy(), yuv_inv_ref(shape, din, dout, pushed),
                     f"yuv420_rgb {din}-{dout}-{shape[0]}x{shape[1]}{'-pushed' if pushed else ''}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [YUV_WRAP_INV, YUV_WRAP_SCALAR, YUV_WRAP_VECTOR],
                         ids=["u16-u8-1032x1024-inverse-wrap", "u8-u8-2056x2056-scalar-wrap", "u8-u8-2056x8192-vector-wrap"])
def test_yuv420_beyond_the_first_sweep(ti, dev, case):
    from taichi_image_amd import _native, color
    shape, din, dout = case
    H, W = shape
    if case is YUV_WRAP_INV:
        got = color.yuv420_rgb_image(_up(dev, yuv_planes_in(shape, din, False)), dtype=dout)
        assert_close(got.cpu().numpy(), yuv_inv_ref(shape, din, dout, False), "yuv420_rgb wrap")
        return
    src = _yuv_in(dev, shape, din)
    got = color.rgb_yuv420_image(src, dtype=dout)
    route = "vector" if _native.rgb_to_yuv420_is_vector(src.data_ptr(), got.data_ptr(), H, W, CODE[dout]) else "scalar"
    assert route == YUV_ROUTE[shape][dout]
    assert_close(got.cpu().numpy(), yuv_fwd_ref(shape, din, dout), f"rgb_yuv420 wrap {route}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", RESIZE_CASES, ids=resize_id)
def test_resize_instances(ti, dev, case):
    """All 16 pairs down (0.8) and up (1.7); a per-axis scale; a requested size two pixels beyond int(scale * src), whose
    last rows and columns clamp both taps to the edge."""
    (din, dout), scale, extra = case
    size = resize_size(RESIZE_SRC, scale, extra)
    got = ti.interpolate.resize_bilinear(_up(dev, resize_src(RESIZE_SRC, din)), size, scale, dtype=tok(ti, dout))
    assert tuple(got.shape) == (size[1], size[0], 3)
    assert_exact(got.cpu().numpy(), resize_ref(RESIZE_SRC, din, dout, scale, extra), f"resize {resize_id(case)}")


@pytest.mark.gpu
def test_resize_beyond_the_first_sweep(ti, dev):
    src, scale, din, dout = RESIZE_WRAP
    got = ti.interpolate.resize_bilinear(_up(dev, resize_src(src, din)), resize_size(src, scale), scale, dtype=tok(ti, dout))
    assert_exact(got.cpu().numpy(), resize_ref(src, din, dout, scale, 0), "resize u8-u16-600x640_s1.7-wrap")


@pytest.mark.gpu
@pytest.mark.parametrize("name", O.TRANSFORMS)
@pytest.mark.parametrize("dt", DT)
def test_transform_instances(ti, dev, dt, name):
    shape = TRANSVERSE_SHAPE if name == "transverse" else TRANSFORM_SHAPE
    src = image_of(shape, dt)
    got = ti.interpolate.transform(_up(dev, src), ti.ImageTransform(name))
    assert_exact(got.cpu().numpy(), O.transform(src, name), f"transform {dt}-{dt}-{shape[0]}x{shape[1]}-{name}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt,name", TRANSFORM_WRAP, ids=lambda v: v)
def test_transform_beyond_the_first_sweep(ti, dev, dt, name):
    src = image_of(WRAP_IMAGE, dt)
    got = ti.interpolate.transform(_up(dev, src), ti.ImageTransform(name))
    assert_exact(got.cpu().numpy(), O.transform(src, name), f"transform {dt} {name} wrap")


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0, 1, 2, 3])
@pytest.mark.parametrize("dt", DT)
def test_rgb_to_bayer_instances(ti, dev, dt, p):
    src = image_of(MOSAIC_SHAPE, dt)
    got = ti.bayer.rgb_to_bayer(_up(dev, src), ti.BayerPattern(p))
    assert_exact(got.cpu().numpy(), O.rgb_to_bayer(src, p), f"rgb_to_bayer {dt}-{dt}-34x36-pattern{p}")


@pytest.mark.gpu
def test_rgb_to_bayer_beyond_the_first_sweep(ti, dev):
    src = image_of(WRAP_IMAGE, "u16")
    got = ti.bayer.rgb_to_bayer(_up(dev, src), ti.BayerPattern(1))
    assert_exact(got.cpu().numpy(), O.rgb_to_bayer(src, 1), "rgb_to_bayer u16 pattern 1 wrap")


def _packed_id(c):
    return f"u8-{c[0]}-{'scaled' if c[1] else 'direct'}-{'ids' if c[2] else 'std'}"


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1], ids=["fast", "bytes"])
@pytest.mark.parametrize("case", PACKED_CASES, ids=_packed_id)
def test_decode12_instances(ti, dev, case, off):
    """4 dtypes x scaled x IDS on the fast path (groups of 4 pairs and a scalar tail) and on a view one byte into its
    buffer (one pair per lane, byte loads).  u8 direct: the low byte of the 12-bit value, as the reference's integer
    narrowing gives it."""
    dt, scaled, ids = case
    enc = packed_bytes(D12_PAIRS * 3 + off, 1)
    view = _up(dev, enc)[off:]
    assert view.data_ptr() % 4 == off
    got = ti.packed.decode12(view, tok(ti, dt), scaled=scaled, ids_format=ids)
    assert_exact(got.cpu().numpy(), O.decode12(enc[off:], dt, scaled, ids), f"decode12 {_packed_id(case)} +{off}")


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 2], ids=["fast", "bytes"])
@pytest.mark.parametrize("dt,scaled", [(dt, s) for dt in DT for s in (False, True)])
def test_decode16_instances(ti, dev, dt, scaled, off):
    enc = packed_bytes(D16_N * 2 + off, 2)
    view = _up(dev, enc)[off:]
    assert view.data_ptr() % 16 == off
    with np.errstate(over="ignore"):                         # (f16 direct: codes above 65504 are inf on both sides)
        ref = O.decode16(enc[off:], dt, scaled)
    got = ti.packed.decode16(view, tok(ti, dt), scaled=scaled)
    assert_exact(got.cpu().numpy(), ref, f"decode16 u8-{dt}-{'scaled' if scaled else 'direct'} +{off}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: f"{c[0]}-u8-{'scaled' if c[1] else 'direct'}-{'ids' if c[2] else 'std'}")
def test_encode12_instances(ti, dev, case):
    dt, scaled, ids = case
    v = encode_values(2 * E12_PAIRS, dt, scaled)
    got = ti.packed.encode12(_up(dev, v), scaled=scaled, ids_format=ids)
    assert_exact(got.cpu().numpy(), O.encode12(v, scaled, ids), f"encode12 {dt} scaled={scaled} ids={ids}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["decode12", "decode12_bytes", "decode16", "encode12"])
def test_packed_beyond_the_first_sweep(ti, dev, which):
    if which == "decode12":
        dt, scaled, ids, pairs = D12_WRAP
        enc = packed_bytes(pairs * 3, 12)
        got = ti.packed.decode12(_up(dev, enc), tok(ti, dt), scaled=scaled, ids_format=ids)
        ref = O.decode12(enc, dt, scaled, ids)
    elif which == "decode12_bytes":
        dt, scaled, ids, pairs = D12_WRAP_BYTES
        enc = packed_bytes(pairs * 3 + 1, 13)
        view = _up(dev, enc)[1:]
        assert view.data_ptr() % 4 == 1
        got = ti.packed.decode12(view, tok(ti, dt), scaled=scaled, ids_format=ids)
        ref = O.decode12(enc[1:], dt, scaled, ids)
    elif which == "decode16":
        dt, scaled, n = D16_WRAP
        enc = packed_bytes(n * 2, 16)
        got = ti.packed.decode16(_up(dev, enc), tok(ti, dt), scaled=scaled)
        ref = O.decode16(enc, dt, scaled)
    else:
        dt, scaled, ids, pairs = E12_WRAP
        v = encode_values(2 * pairs, dt, scaled)
        got = ti.packed.encode12(_up(dev, v), scaled=scaled, ids_format=ids)
        ref = O.encode12(v, scaled, ids)
    assert_exact(got.cpu().numpy(), ref, f"{which} wrap")


def _load_convert(dev, mode, dout, n):
    import torch
    from taichi_image_amd import _native
    src = _up(dev, lc_src(mode, n))
    dst = torch.empty(n, dtype=_torch_dtype(dout), device=dev)
    _native.check(_native.lib().mi_isp_load_convert(src.data_ptr(), dst.data_ptr(), n, LC_MODES[mode][0], CODE[dout],
                                                    _native.stream_ptr(dev)))
    torch.cuda.synchronize()
    return dst.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dout", ["f16", "f32"])
@pytest.mark.parametrize("mode", list(LC_MODES))
def test_load_convert_instances(ti, dev, mode, dout):
    """mi_isp_load_convert alone (the ISP's loaders put a demosaic behind it): 3 modes x 2 outputs."""
    assert_exact(_load_convert(dev, mode, dout, LC_N), LC_MODES[mode][1](lc_src(mode, LC_N), dout), f"load_convert {mode}-{dout}")


@pytest.mark.gpu
def test_load_convert_beyond_the_first_sweep(ti, dev):
    mode, dout, n = LC_WRAP
    assert_exact(_load_convert(dev, mode, dout, n), LC_MODES[mode][1](lc_src(mode, n), dout), "load_convert 16u-f16 wrap")
