"""The directional demosaic (csrc/isp_demosaic_dir.hip) and the antialiased resize (csrc/isp_resample.hip) at their
limits, and the two options through every loader route, bit for bit against the restatements the tree has
(tests/demosaic_ref.py; tests/resample_ref.py fed with the library's own tables).

A. The resize kernel.
   1. T = 32 on both axes for each filter and T = 29 (the first ring capped at MAX_TAPS + ROWS rows): the geometries of
      LIMITS, whose tap counts a CPU test asserts on the library's and the restatement's tables; a second CPU test restates
      lds_bytes() from the constants of isp_resample.h: Tx = Ty = 32 with an f32 source is the largest block and fits 64 KiB.
   2. The 16-byte-unit staging at SEG_PX: crafted column tables whose first tile spans exactly 512 source pixels (the LDS
      segment filled to its last unit on a row that starts off a 16-byte boundary), whose second spans 513 (the first span
      read from memory) and whose third ends on the last element of the image's last row (the tail unit copied element by
      element); the rows of the 1051-pixel source walk through every residue; once more one element into a larger buffer.
   3. The ring / from-memory fork: crafted row tables whose first tile row has the widest window the ring holds
      (ring_rows - ROWS + 1: 9 at Ty = 5, 33 at Ty = 32) and whose second has one more, so one launch mixes ring tiles and
      memory tiles; Wd = 65 gives each a one-column neighbour.  ready, lowest and the window are computed here as the
      kernel's comment defines them and asserted before the launch.  Both windows sit where the step that completes their
      output row has filtered ROWS - 1 rows beyond it, the ring at its fullest: elsewhere a ring one row short holds them.
   4. 33 images in one call (MAX_IMAGES = 32: the second launch), distinct contents, sentinels between the destinations.
B. The demosaic kernels' element-by-element stores: the output a view one element into a sentinel-filled buffer (u8 at an
   odd byte, u16 / f16 at 2 mod 4, the f32 CFA at 4 mod 8) through the three C entry points: the aligned call's bits, the
   restatement's, and the sentinels stay.  (tests/test_demosaic_cpu.py holds the refusal of a pointer that is not aligned
   to its element.)
C. The options through the loaders of Camera16 and Camera32 at 66 x 70 -> 30 x 32 (scale 32 / 70 suits all three filters):
   every loader kind with the resize alone and with both options (single and batch surface), the chains MH, MC, MD, CT, HT
   and TD of the raw-stage matrix with the demosaic alone, the resize alone and both (one chain per camera with a lens),
   auto white balance, set() between two loads of one temporal history, and process_packed12.  The reference is composed:
   the CFA of the route (pinned by the raw-stage matrix), the demosaic's restatement or the oracle's 13-tap filter, the
   lens remap of an ISP without the options (pinned by its own files), the resize's restatement or the oracle's bilinear.

The first tests need no GPU.  profiles/demosaic_resample_matrix_mutations.txt records the deliberate edits of the library
these tests were run against."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

from oracle import isp_oracle as O
from tests import demosaic_ref as R
from tests import denoise_ref as D
from tests import resample_ref as RS
from tests import test_gpu_resample as RC
from tests.test_defects_cpu import correct_cfa
from tests.test_gpu_demosaic import CCM, raw_call, route_cfa, source
from tests.test_gpu_raw_stage_matrix import (CAMS, CHAINS, ENTRY, KINDS, PACKED, SEAMS, call, capture, cfa_of, chain_case,
                                             chain_settings, grid, load_bracket, record_outputs, the_map, to_dev)
from tests.test_gpu_resample import NP, PAIRS, assert_same, cast
from tests.test_gpu_shading import pixel_gains
from tests.util import _count_calls, assert_exact

gpu = pytest.mark.gpu
f32 = np.float32
FILTERS = RS.FILTERS
OUTS = ["u8", "u16", "f16", "f32"]
SENTINEL = -7.0

# the constants of csrc/isp_resample.h (test_lds_bytes_at_the_limit reads them from the source)
OW, OH, ROWS, SEG_PX, MAX_TAPS, MAX_IMAGES = 64, 32, 4, 512, 32, 32
THREADS = OW * 3

# A1: (filter, Hs, Ws, Hd, Wd, scale, T on both axes)
LIMITS = [("lanczos3", 200, 70, 38, 13, 3 / 16, 32), ("triangle", 200, 70, 13, 5, 0.064, 32),
          ("area", 200, 100, 7, 3, 0.0325, 32), ("lanczos3", 70, 70, 14, 14, 0.2, 29)]
N_IMAGES = 33

# C: the resize of every case, the option sets and the tables of the cases
RW = 32
OPTION_SETS = ["dm", "aa", "both"]
FILTER_OF = {k: FILTERS[i % 3] for i, k in enumerate(KINDS)}            # each filter meets a packed and an unpacked kind
LOADER_CASES = [(k, o) for k in KINDS for o in ("aa", "both")]
OPTION_CHAINS = ["MH", "MC", "MD", "CT", "HT", "TD"]
CHAIN_OPTION_CASES = [(c, k, o) for c in OPTION_CHAINS for k in ("p12", CHAINS[c]) for o in OPTION_SETS]
LENS_CHAIN = {"Camera16": ("HT", "p12"), "Camera32": ("MC", "p12")}      # the chain of a camera that carries a lens


def _rng(*key):
    return np.random.default_rng([20262, *[int(k) for k in key]])


def _ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def ti():
    return _ti()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def random_image(rng, H, W, work):
    """Random values in [-1, 3), as tests/test_gpu_resample.py draws them."""
    return (rng.random((H, W, 3), dtype=f32) * 4 - 1).astype(NP[work])


def random_axis(rng, start, T):
    """A crafted table of an axis: the given starts, random normal weights."""
    start = np.asarray(start, dtype=np.int32)
    return T, start, rng.standard_normal((len(start), T)).astype(f32)


def ring_rows_of(Ty):
    return min(Ty + ROWS - 1 + 4, MAX_TAPS + ROWS)


def lds_bytes(Ty, Tx, size):
    """rs::lds_bytes restated: ROWS segments, the ring, the two weight tables, starts / slot / ready / lowest / extents."""
    return ROWS * (SEG_PX * 3 * size + 16) + ring_rows_of(Ty) * THREADS * 4 + OW * Tx * 4 + OH * Ty * 4 + (OW + 4 * OH + 5) * 4


def spans_of(start, T):
    """Per tile of OW output columns: max(start + T) - min(start), what the kernel compares with SEG_PX."""
    return [int(start[x0:x0 + OW].max()) + T - int(start[x0:x0 + OW].min()) for x0 in range(0, len(start), OW)]


def windows_of(start, T):
    """Per tile of OH output rows the kernel's ext[4]: ready is the prefix maximum of start + T, lowest the suffix minimum
    of start, the window the largest ready - lowest."""
    out = []
    for y0 in range(0, len(start), OH):
        s = start[y0:y0 + OH].astype(np.int64)
        ready = np.maximum.accumulate(s + T)
        lowest = np.minimum.accumulate(s[::-1])[::-1]
        out.append(int((ready - lowest).max()))
    return out


def rows_ahead_of(start, T):
    """Per tile of OH output rows, at its widest window: the most source rows the step that completes such an output row
    has filtered beyond it (the kernel walks the rows from the tile's first in steps of ROWS): ROWS - 1 is the ring at
    its fullest."""
    out = []
    for y0 in range(0, len(start), OH):
        s = start[y0:y0 + OH].astype(np.int64)
        ready = np.maximum.accumulate(s + T)
        window = ready - np.minimum.accumulate(s[::-1])[::-1]
        out.append(max(int(-(r - s.min()) % ROWS) for r in ready[window == window.max()]))
    return out


def rising(rng, lo, hi, n):
    """n rising starts, the first lo, the last hi."""
    return np.concatenate([[lo], np.sort(rng.integers(lo, hi + 1, n - 2)), [hi]])


@functools.lru_cache(maxsize=None)
def segment_tables():
    """A2: (Hs, Ws, Hd, Wd, rows, cols)."""
    rng = _rng(2)
    Hs, Ws, Hd, Wd, Ty, Tx = 9, 1051, 5, 130, 3, 4
    sx = np.concatenate([rising(rng, 3, 3 + SEG_PX - Tx, OW), rising(rng, 300, 300 + SEG_PX + 1 - Tx, OW),
                         [Ws - Tx - 7, Ws - Tx]])
    return Hs, Ws, Hd, Wd, random_axis(rng, [0, 1, 3, 5, Hs - Ty], Ty), random_axis(rng, sx, Tx)


@functools.lru_cache(maxsize=None)
def fork_tables(Ty):
    """A3: (Hs, Ws, Hd, Wd, rows, cols) for Ty = 5 or 32: the first tile row's window is the widest the ring holds, the
    second's one more."""
    rng = _rng(3, Ty)
    Hs, Ws, Hd, Wd, Tx = {5: 60, 32: 120}[Ty], 150, 40, 65, 3
    hold = ring_rows_of(Ty) - ROWS + 1
    # a row whose start falls back behind the rows before it widens the window.  The row in front of it completes one
    # source row into a step of ROWS (ready - the tile's first row = 1 mod ROWS), so the step that completes it has brought
    # ROWS - 1 rows more and the ring is at its fullest when the window is read
    j = {5: 20, 32: 21}[Ty]
    first = np.arange(OH)
    first[j + 1] = (j + Ty) - hold                       # ready[j] - start[j + 1] = hold
    base = {5: 40, 32: 50}[Ty]
    second = base + np.array({5: [0, 2, 5, 8, 3, 9, 10, 0], 32: [0, 1, 2, 5, 3, 6, 7, 0]}[Ty])
    assert second[3] + Ty - second[4] == hold + 1
    second[-1] = Hs - Ty                                 # (the last source row is read)
    sx = rising(rng, 0, Ws - Tx, Wd)
    return Hs, Ws, Hd, Wd, random_axis(rng, np.concatenate([first, second]), Ty), random_axis(rng, sx, Tx)


_planes: dict = {}


def planes(cfa, pattern):
    """R.planes of a CFA, computed once per (frame, pattern) and shared; never written."""
    key = (cfa.shape, str(cfa.dtype), cfa.tobytes(), int(pattern))
    if key not in _planes:
        _planes[key] = R.planes(cfa, pattern)
        _planes[key].setflags(write=False)
    return _planes[key]


# ---- without a GPU: the tables -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt,Hs,Ws,Hd,Wd,s,T", LIMITS)
def test_the_limit_geometries_reach_their_taps(filt, Hs, Ws, Hd, Wd, s, T):
    """The library's and the restatement's tables of A1 have exactly these tap counts on both axes, their starts rise and
    the first and the last tap carry a non-zero weight somewhere."""
    from taichi_image_amd import resample as rs
    assert T in (29, MAX_TAPS)
    for S, Dn in ((Hs, Hd), (Ws, Wd)):
        assert rs.taps(filt, S, Dn, s) == T
        t_lib, start, weight = rs.table(filt, S, Dn, s)
        t_ref, start_ref, weight_ref = RS.table(filt, S, Dn, s)
        assert t_lib == T and t_ref == T
        assert np.array_equal(start, start_ref) and (np.diff(start) >= 0).all()
        assert start.min() >= 0 and start.max() + T <= S
        assert (weight[:, 0] != 0).any() and (weight[:, -1] != 0).any()
        assert (weight_ref[:, 0] != 0).any() and (weight_ref[:, -1] != 0).any()
    assert ring_rows_of(T) == MAX_TAPS + ROWS and ring_rows_of(28) < MAX_TAPS + ROWS
    assert windows_of(rs.table(filt, Hs, Hd, s)[1], T) == [T] * ((Hd + OH - 1) // OH), "a rising table: the ring"


def test_lds_bytes_at_the_limit():
    """The constants this file assumes are the source's, and the largest block - Tx = Ty = 32, an f32 source - fits the
    64 KiB a block gets."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "taichi_image_amd", "csrc", "isp_resample.h")) as f:
        text = f.read()
    for name, value in (("OW", OW), ("OH", OH), ("ROWS", ROWS), ("SEG_PX", SEG_PX), ("MAX_IMAGES", MAX_IMAGES)):
        found = re.findall(rf"constexpr int {name} = (\d+);", text)
        assert found == [str(value)], f"isp_resample.h: {name} is {found}, the tests assume {value}"
    assert re.findall(r"constexpr int THREADS = OW \* 3;", text) and re.findall(r"constexpr int MAX_TAPS = MI_RESAMPLE_MAX_TAPS;", text)
    with open(os.path.join(root, "include", "mi_isp.h")) as f:
        assert re.findall(r"#define MI_RESAMPLE_MAX_TAPS (\d+)", f.read()) == [str(MAX_TAPS)]
    top = lds_bytes(MAX_TAPS, MAX_TAPS, 4)
    assert top == 65364 and top <= 65536
    sizes = {(ty, tx, size): lds_bytes(ty, tx, size) for ty in range(1, MAX_TAPS + 1) for tx in range(1, MAX_TAPS + 1)
             for size in (2, 4)}
    assert max(sizes.values()) == top and [k for k, v in sizes.items() if v == top] == [(MAX_TAPS, MAX_TAPS, 4)]
    # the ring holds a window of ring_rows - ROWS + 1 rows: Ty + 4 below the cap, then down to Ty + 1 at Ty = 32
    assert [ring_rows_of(t) - ROWS + 1 - t for t in (1, 5, 28, 29, 30, 31, 32)] == [4, 4, 4, 4, 3, 2, 1]
    assert N_IMAGES > MAX_IMAGES


def test_the_segment_tables_hold_512_513_and_the_last_element():
    Hs, Ws, Hd, Wd, rows, cols = segment_tables()
    Tx, sx, _ = cols
    assert len(sx) == Wd == 2 * OW + 2 and (np.diff(sx[:OW]) >= 0).all() and (np.diff(sx[OW:2 * OW]) >= 0).all()
    assert spans_of(sx, Tx)[:2] == [SEG_PX, SEG_PX + 1] and spans_of(sx, Tx)[2] <= SEG_PX
    assert sx.min() >= 0 and sx[-1] == Ws - Tx == sx.max(), "the third tile ends on the row's last pixel"
    assert rows[1][-1] + rows[0] == Hs, "... and the last output row reads the last source row"
    assert sx[:OW].min() * 3 * 2 % 16 != 0 and sx[:OW].min() * 3 * 4 % 16 != 0, "tile 0 starts off a 16-byte boundary"
    for size in (2, 4):
        assert Ws * 3 * size % 16 == size, "the rows walk through the residues"
        # a row of tile 0 whose segment starts `off` bytes into its first unit fills the LDS segment to its last unit
        seg = SEG_PX * 3 * size
        offs = {(r * Ws + int(sx[:OW].min())) * 3 * size % 16 for r in range(Hs)}
        assert max((seg + off + 15) // 16 * 16 for off in offs) == seg + 16, "n_units * 16 == SEG on some row"
    assert windows_of(rows[1], rows[0]) == [rows[0]], "the ring"


@pytest.mark.parametrize("Ty", [5, 32])
def test_the_fork_tables_sit_on_both_sides_of_the_threshold(Ty):
    Hs, Ws, Hd, Wd, rows, cols = fork_tables(Ty)
    hold = ring_rows_of(Ty) - ROWS + 1
    assert hold == {5: 9, 32: 33}[Ty]
    sy = rows[1]
    assert sy.min() >= 0 and sy.max() + Ty == Hs and len(sy) == Hd and Hd > OH
    assert windows_of(sy, Ty) == [hold, hold + 1], "a ring tile row and a from-memory tile row in one launch"
    # both windows meet the ring at its fullest: a ring one row short, or a threshold one row up, loses their oldest row
    assert rows_ahead_of(sy, Ty) == [ROWS - 1, ROWS - 1]
    assert all(sy[y0:y0 + OH].max() + Ty - sy[y0:y0 + OH].min() > hold + 1 + ROWS for y0 in (0, OH)), "the ring wraps"
    assert Wd == OW + 1 and spans_of(cols[1], cols[0])[0] <= SEG_PX


def test_the_option_cases_are_the_full_cross_products():
    assert LOADER_CASES == list(itertools.product(KINDS, ("aa", "both"))) and len(set(LOADER_CASES)) == 12
    assert KINDS == ["p12", "ids", "p16", "16u", "16f", "32f"] and OPTION_SETS == ["dm", "aa", "both"]
    for filt in FILTERS:
        kinds = [k for k in KINDS if FILTER_OF[k] == filt]
        assert len(kinds) == 2 and (kinds[0] in PACKED) != (kinds[1] in PACKED)
    assert CHAIN_OPTION_CASES == [(c, k, o) for c in OPTION_CHAINS for k in ("p12", CHAINS[c]) for o in OPTION_SETS]
    assert len(set(CHAIN_OPTION_CASES)) == 6 * 2 * 3 and all(k != "p12" for k in (CHAINS[c] for c in OPTION_CHAINS))
    assert {k for _, k, _ in CHAIN_OPTION_CASES} == set(KINDS), "every kind behind some chain"
    assert all((c, k, o) in CHAIN_OPTION_CASES for c, k in LENS_CHAIN.values() for o in OPTION_SETS)
    assert sorted(LENS_CHAIN) == [c for c, _ in CAMS] and all("M" in c or "T" in c for c, _ in LENS_CHAIN.values())
    H, W = SEAMS
    for filt in FILTERS:                                   # the scale suits every filter
        assert RS.table(filt, W, RW, RW / W)[0] <= MAX_TAPS and RS.table(filt, H, round(H * RW / W), RW / W)[0] <= MAX_TAPS
    # the parametrisation of the GPU tests is these tables
    marks = {m.args[0]: m.args[1] for m in test_every_loader_with_the_options.pytestmark if m.name == "parametrize"}
    assert marks["kind,opts"] is LOADER_CASES and marks["cam,work"] is CAMS
    marks = {m.args[0]: m.args[1] for m in test_chains_with_the_options.pytestmark if m.name == "parametrize"}
    assert marks["chain,kind,opts"] is CHAIN_OPTION_CASES and marks["cam,work"] is CAMS
    marks = {m.args[0]: m.args[1] for m in test_taps_at_the_limit.pytestmark if m.name == "parametrize"}
    assert marks["filt,Hs,Ws,Hd,Wd,s,T"] is LIMITS and marks["tin,tout"] is PAIRS


# ---- A. the resize kernel at its limits --------------------------------------------------------------------------------
def resample_call(srcs, dsts, Hs, Ws, Hd, Wd, rows, cols, tin, tout, dev):
    """mi_isp_resample_batch on device tensors with the host tables rows and cols."""
    from taichi_image_amd import _native, types
    held = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rows[1], rows[2], cols[1], cols[2])]
    ax = [_native.ResampleAxis(rows[0], held[0].data_ptr(), held[1].data_ptr()),
          _native.ResampleAxis(cols[0], held[2].data_ptr(), held[3].data_ptr())]
    _native.check(_native.lib().mi_isp_resample_batch(
        _native.ptr_array(srcs), _native.ptr_array(dsts), len(srcs), Hs, Ws, Hd, Wd, types.as_dtype(tin).code,
        types.as_dtype(tout).code, ctypes.byref(ax[0]), ctypes.byref(ax[1]), _native.stream_ptr(dev)))
    torch.cuda.synchronize(dev)


@gpu
@pytest.mark.parametrize("tin,tout", PAIRS)
@pytest.mark.parametrize("filt,Hs,Ws,Hd,Wd,s,T", LIMITS)
def test_taps_at_the_limit(ti, dev, filt, Hs, Ws, Hd, Wd, s, T, tin, tout):
    from taichi_image_amd import resample as rs
    src = random_image(_rng(1, LIMITS.index((filt, Hs, Ws, Hd, Wd, s, T)), tin == "f32"), Hs, Ws, tin)
    rows, cols = rs.table(filt, Hs, Hd, s), rs.table(filt, Ws, Wd, s)
    assert rows[0] == T and cols[0] == T
    want = cast(RS.resample(src, rows, cols, f32), tout)
    got = ti.interpolate.resample(to_dev(src, dev), (Wd, Hd), s, filt, dtype=tout)
    assert_same(got.cpu().numpy(), want, f"{filt} T={T} {Hs}x{Ws} -> {Hd}x{Wd} {tin}->{tout}")


@gpu
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("work", ["f16", "f32"])
def test_the_segment_at_512_and_513_source_pixels(ti, dev, work, offset):
    """offset 1: the source a contiguous view one element into a larger buffer."""
    Hs, Ws, Hd, Wd, rows, cols = segment_tables()
    assert spans_of(cols[1], cols[0])[:2] == [SEG_PX, SEG_PX + 1]
    src = random_image(_rng(4, work == "f32"), Hs, Ws, work)
    want = RS.resample(src, rows, cols, NP[work])
    n = src.size
    whole = torch.zeros(n + (9 if offset else 0), dtype=torch.from_numpy(src).dtype, device=dev)
    view = whole[offset:offset + n].view(Hs, Ws, 3)
    view.copy_(torch.from_numpy(src))
    assert view.is_contiguous() and view.data_ptr() == whole.data_ptr() + offset * whole.element_size()
    out = torch.full((Hd, Wd, 3), SENTINEL, dtype=whole.dtype, device=dev)
    resample_call([view], [out], Hs, Ws, Hd, Wd, rows, cols, work, work, dev)
    assert_same(out.cpu().numpy(), want, f"{work} offset {offset}")


@gpu
@pytest.mark.parametrize("tin,tout", PAIRS)
@pytest.mark.parametrize("Ty", [5, 32])
def test_ring_tiles_and_memory_tiles_in_one_launch(ti, dev, Ty, tin, tout):
    Hs, Ws, Hd, Wd, rows, cols = fork_tables(Ty)
    hold = ring_rows_of(Ty) - ROWS + 1
    assert windows_of(rows[1], Ty) == [hold, hold + 1]
    src = random_image(_rng(5, Ty, tin == "f32"), Hs, Ws, tin)
    want = cast(RS.resample(src, rows, cols, f32), tout)
    out = torch.full((Hd, Wd, 3), SENTINEL, dtype=torch.from_numpy(want).dtype, device=dev)
    resample_call([to_dev(src, dev)], [out], Hs, Ws, Hd, Wd, rows, cols, tin, tout, dev)
    got = out.cpu().numpy()
    assert_same(got[:OH], want[:OH], f"Ty={Ty} {tin}->{tout}: the tile row of window {hold} (the ring)")
    assert_same(got[OH:], want[OH:], f"Ty={Ty} {tin}->{tout}: the tile row of window {hold + 1} (from memory)")


@gpu
@pytest.mark.parametrize("tin,tout", PAIRS)
def test_33_images_in_one_call(ti, dev, monkeypatch, tin, tout):
    """More images than one launch takes: every image is its own reference, and nothing between the destinations - views
    into one sentinel-filled buffer - changes."""
    from taichi_image_amd import resample as rs
    from taichi_image_amd import types
    filt = FILTERS[PAIRS.index((tin, tout)) % 3]
    n_calls = _count_calls(monkeypatch, "mi_isp_resample_batch")
    for case in ("small", "tile+1"):
        Hs, Ws, Hd, Wd, s0, s1 = RC.CASES[case]
        srcs = [to_dev(RC.source(case, tin, k), dev) for k in range(N_IMAGES)]
        n, pad = Hd * Wd * 3, 5
        whole = torch.full((pad + N_IMAGES * (n + pad),), SENTINEL, dtype=types.as_dtype(tout).torch, device=dev)
        at = [pad + k * (n + pad) for k in range(N_IMAGES)]
        dsts = [whole[a:a + n].view(Hd, Wd, 3) for a in at]
        n_calls.clear()
        rs.apply(srcs, dsts, filt, Hs, Ws, Hd, Wd, s0, s1, types.as_dtype(tin).code, types.as_dtype(tout).code, dev)
        assert len(n_calls) == 1
        host = whole.cpu().numpy()
        wants = [cast(RC.reference(case, filt, tin, k), tout) for k in range(N_IMAGES)]
        assert len({w.tobytes() for w in wants}) == N_IMAGES, "every image has content of its own"
        between = np.ones(host.size, bool)
        for k, a in enumerate(at):
            assert_same(host[a:a + n].reshape(Hd, Wd, 3), wants[k], f"{filt} {case} {tin}->{tout} image {k} of {N_IMAGES}")
            between[a:a + n] = False
        assert_exact(host[between], np.full(int(between.sum()), SENTINEL, host.dtype), f"{case}: between the destinations")


# ---- B. the demosaic kernels' element-by-element stores ----------------------------------------------------------------
def one_off(shape, out, dev):
    """(whole, view): a sentinel-filled buffer one element longer at each end than `shape`, and the view one element in."""
    n = int(np.prod(shape))
    fill = 7 if out in ("u8", "u16") else SENTINEL
    whole = torch.from_numpy(np.full(n + 2, fill, dtype=O.NP_DTYPE[out])).to(dev)
    view = whole[1:1 + n].view(*shape)
    size = whole.element_size()
    assert view.is_contiguous() and view.data_ptr() == whole.data_ptr() + size and whole.data_ptr() % 16 == 0
    return whole, view, fill


def assert_ends_stay(whole, fill, what):
    host = whole.cpu().numpy()
    assert host[0] == fill and host[-1] == fill, f"{what}: the elements around the view: {host[0]}, {host[-1]}"


@gpu
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("out", OUTS)
def test_directional_cfa_into_a_view_one_element_off(ti, dev, work, out):
    """store6's element-by-element route: u8 at an odd byte, u16 / f16 at 2 mod 4 (an f32 image one element off is still
    on a dword: the vector route at 4 mod 8)."""
    from taichi_image_amd import _native, types
    L, stream = _native.lib(), _native.stream_ptr(dev)
    for k, shape in enumerate([R.SHAPES[-1], (2, 6)]):
        H, W = shape
        pattern = (k + OUTS.index(out)) % 4
        cfa = R.stripes_cfa(shape, k, O.NP_DTYPE[work])
        want = R.finish(planes(cfa, pattern), CCM, out)
        t = to_dev(cfa, dev)
        aligned = torch.from_numpy(np.zeros(shape + (3,), dtype=O.NP_DTYPE[out])).to(dev)
        whole, view, fill = one_off(shape + (3,), out, dev)
        size = whole.element_size()
        assert view.data_ptr() % (2 if size == 1 else 4) == size % 4 and aligned.data_ptr() % 16 == 0
        for dst in (aligned, view):
            _native.check(L.mi_isp_demosaic_directional_cfa(t.data_ptr(), dst.data_ptr(), H, W, types.as_dtype(work).code,
                                                            types.as_dtype(out).code, pattern, _native.ccm_arg(CCM), stream))
        torch.cuda.synchronize(dev)
        what = f"{work} -> {out} {shape} p{pattern}"
        assert_exact(aligned.cpu().numpy(), want, what + " aligned")
        assert_exact(view.cpu().numpy(), want, what + " one element off")
        assert_ends_stay(whole, fill, what)


@gpu
@pytest.mark.parametrize("work", ["f16", "f32"])
@pytest.mark.parametrize("kind", ["p12", "32f"])
def test_raw_entry_points_into_views_one_element_off(ti, dev, kind, work):
    """mi_isp_demosaic_directional_raw_batch (the f16 image at 2 mod 4) and mi_isp_raw_cfa_batch (the f16 CFA at 2 mod 4,
    the f32 CFA at 4 mod 8: raw_cfa_kernel's two single stores), with levels where the kind takes them and a grid."""
    tdt = torch.float16 if work == "f16" else torch.float32
    g = np.array(grid())
    for k, shape in enumerate([R.SHAPES[-1], (2, 6)]):
        pattern = (k + 1) % 4
        src, x, black, white, ccm = source(kind, shape, k, levels=True)
        cfa = route_cfa(x, g, work)
        t = to_dev(src, dev)
        what = f"{kind} {work} {shape} p{pattern}"
        for name, tail, want in (("rgb", (3,), R.finish(planes(cfa, pattern), ccm, work)), ("cfa", (), cfa)):
            aligned = torch.full(shape + tail, SENTINEL, dtype=tdt, device=dev)
            whole, view, fill = one_off(shape + tail, work, dev)
            size = whole.element_size()
            assert view.data_ptr() % (2 * size) == size and aligned.data_ptr() % 16 == 0
            for dst in (aligned, view):
                raw_call(name, [t], [dst], shape, kind, work, pattern, black, white, g, ccm if name == "rgb" else None, dev)
            assert_exact(aligned.cpu().numpy(), want, f"{what} {name} aligned")
            assert_exact(view.cpu().numpy(), want, f"{what} {name} one element off")
            assert_ends_stay(whole, fill, f"{what} {name}")


# ---- C. the options through every route --------------------------------------------------------------------------------
def options(ti, opts, filt):
    kw = {}
    if opts in ("dm", "both"):
        kw["demosaic"] = ti.Demosaic("directional")
    if opts in ("aa", "both"):
        kw["resample"] = ti.Resample(filt)
    return kw


def resized(rgb, filt):
    """A full-resolution work-dtype image through the restatement at resize_width = RW, on the library's tables."""
    from taichi_image_amd import resample as rs
    h, w = rgb.shape[:2]
    s = RW / w
    return RS.resample(rgb, rs.table(filt, h, round(h * s), s), rs.table(filt, w, RW, s))


def composed(cfa, pattern, ccm, work, opts, filt, remap=None):
    """The image of a route's CFA under an option set: the demosaic (the restatement, or the oracle's 13-tap filter), the
    lens remap (remap(rgb, full): at the frame's own size in front of the antialiased resize, else at the resize
    geometry), the resize (the restatement, or the oracle's bilinear)."""
    H, W = cfa.shape
    aa = opts in ("aa", "both")
    if opts in ("dm", "both"):
        rgb = R.finish(planes(cfa, pattern), ccm, work)
    else:
        rgb = O.bayer_to_rgb(cfa, pattern, correct_colors=ccm)
    if remap is not None:
        rgb = remap(rgb, aa)
    if aa:
        return resized(rgb, filt)
    if remap is not None:
        return rgb
    sz = O.isp_output_size(H, W, RW, None)
    return O.resize_bilinear(rgb, sz[0], sz[1])


def the_lens(ti):
    H, W = SEAMS
    K = np.array([[64.0, 0, W / 2 - 3], [0, 66.0, H / 2 + 2], [0, 0, 1]])
    return ti.LensDistortion(K, (-0.2, 0.05, 0.001, -0.002), SEAMS)


def remap_of(ti, cam, dev, lens):
    """The lens remap of an ISP without the two options (pinned by tests/test_gpu_lens.py)."""
    H, W = SEAMS

    def remap(rgb, full):
        twin = getattr(ti, cam)(ti.BayerPattern.RGGB, device=dev, resize_width=0 if full else RW)
        return twin._undistort([to_dev(rgb, dev)], [lens], H, W)[0].cpu().numpy()
    return remap


def capture_both(monkeypatch, isp):
    """capture(), and the CFAs handed to _process_full in the same list; the names of the routes taken beside it."""
    got = capture(monkeypatch, isp)
    names = []
    cls = type(isp)
    image, full = cls._process_image, cls._process_full

    def process_image(self, cfa, lens=None):
        names.append("_process_image")
        return image(self, cfa, lens)

    def process_full(self, cfa, lens=None):
        names.append("_process_full")
        got.append(cfa.clone())
        return full(self, cfa, lens)

    monkeypatch.setattr(cls, "_process_image", process_image)
    monkeypatch.setattr(cls, "_process_full", process_full)
    return got, names


def batch_call(isp, kind, ts, **kw):
    if kind == "p16":
        return isp.load_packed16_batch(ts, **kw)
    return isp.load_packed12_batch(ts, ids_format=kind == "ids", **kw)


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind,opts", LOADER_CASES)
def test_every_loader_with_the_options(ti, dev, monkeypatch, cam, work, kind, opts):
    """No raw stage: levels where the kind takes them, a grid; the single and - for the packed kinds - the batch surface."""
    H, W = SEAMS
    filt, pattern = FILTER_OF[kind], KINDS.index(kind) % 4
    frames = [source(kind, SEAMS, k, levels=True) for k in range(3 if kind in PACKED else 1)]
    black, white, ccm = frames[0][2:5]
    g = np.array(grid())
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, color_correction=np.array(ccm),
                           black_level=black, white_level=white, lens_shading=g, resize_width=RW, **options(ti, opts, filt))
    want = [composed(route_cfa(f[1], g, work), pattern, isp.color_correct_matrix, work, opts, filt) for f in frames]
    assert want[0].shape == (round(H * RW / W), RW, 3)
    ts = [to_dev(f[0], dev) for f in frames]
    n_rs = _count_calls(monkeypatch, "mi_isp_resample_batch")
    n_dir = _count_calls(monkeypatch, "mi_isp_demosaic_directional_raw_batch")
    n_bil = _count_calls(monkeypatch, "mi_isp_resize_bilinear")
    what = f"{cam} {kind} {opts} {filt}"
    img = call(isp, kind, ts[0])
    assert getattr(img, "_mi_metering_sub", None) is None
    assert_exact(img.cpu().numpy(), want[0], what + " single")
    assert len(n_rs) == 1 and not n_bil
    if kind in PACKED:
        assert len(n_dir) == (opts == "both")
        n_rs.clear(), n_dir.clear()
        imgs = batch_call(isp, kind, ts)
        assert len(n_rs) == 1 and len(n_dir) == (opts == "both") and not n_bil, "ONE launch each for the batch"
        for k in range(len(ts)):
            assert_exact(imgs[k].cpu().numpy(), want[k], f"{what} batch image {k}")
        assert len({w.tobytes() for w in want}) == len(want)


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("chain,kind,opts", CHAIN_OPTION_CASES)
def test_chains_with_the_options(ti, dev, monkeypatch, cam, work, chain, kind, opts):
    """test_chain_positions of the raw-stage matrix with the options on: everything in front of the demosaic as there, the
    image composed from the route's CFA."""
    H, W = SEAMS
    c = chain_case(chain, kind)
    st, mask, pattern = c["settings"], c["mask"], c["pattern"]
    assert set(st) == set(chain_settings(chain, kind))
    m = the_map(H, W)
    filt = FILTERS[(OPTION_CHAINS.index(chain) + (kind != "p12")) % 3]
    lens = the_lens(ti) if LENS_CHAIN[cam] == (chain, kind) else None
    remap = None if lens is None else remap_of(ti, cam, dev, lens)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), device=dev, correct_colors=True, black_level=c["black"],
                           white_level=c["white"], lens_shading=np.array(grid()), exposure_merge=st.get("M"),
                           highlights=st.get("H"), chromatic_aberration=st.get("C"), temporal_denoise=st.get("T"),
                           raw_denoise=st.get("D"), resize_width=RW, **options(ti, opts, filt))
    wrote = {s: record_outputs(monkeypatch, *ENTRY[s]) for s in chain[:-1]}
    counts = {s: _count_calls(monkeypatch, ENTRY[s][0]) for s in "MHCTD"}
    got, names = capture_both(monkeypatch, isp)
    hist = ti.TemporalHistory() if "T" in chain else None
    kw = dict(defects=m)
    if hist is not None:
        kw["history"] = hist
    if lens is not None:
        kw["undistort"] = lens
    # the packed loaders leave the resize to one launch behind _process_full; every other loader resizes in _process_image
    route = "_process_full" if opts in ("aa", "both") and kind in PACKED else "_process_image"
    for k, step in enumerate(c["steps"]):
        what = f"{cam} {chain} {kind} {opts} {filt} load {k}"
        got.clear(), names.clear()
        srcs = [to_dev(a, dev) for a in step["srcs"]]
        img = (load_bracket(isp, kind, srcs, **kw) if "M" in chain else call(isp, kind, srcs[0], **kw)).cpu().numpy()
        for s in chain[:-1]:                               # every stage in front of the last: its plain f32 y
            assert len(wrote[s]) == k + 1 and len(wrote[s][k]) == 1
            assert_exact(wrote[s][k][0].cpu().numpy(), step["ys"][s], f"{what}: the plain y of {s}")
        if hist is not None:
            assert hist.frames == k + 1
            assert_exact(hist.plane.cpu().numpy(), step["ys"]["T"], f"{what}: the temporal history")
        assert len(got) == 1 and names == [route], names
        cfa = got[0].cpu().numpy()
        if chain[-1] == "D":
            yg = D.route_yg(step["inputs"]["D"], st["D"], pixel_gains(grid(), H, W), mask)
            D.assert_within_bound(cfa, yg, work, what, where=~mask)
            assert_exact(cfa, correct_cfa(cfa, mask, work), what + ": the defect fix-up")
        else:
            assert_exact(cfa, cfa_of(isp, step["ys"][chain[-1]], work, mask), what + " CFA")
        assert_exact(img, composed(cfa, pattern, isp.color_correct_matrix, work, opts, filt, remap), what + " image")
    assert {s: len(n) for s, n in counts.items()} == {s: len(c["steps"]) if s in chain else 0 for s in "MHCTD"}


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "16u"])
def test_auto_white_balance_with_both_options(ti, dev, monkeypatch, cam, work, kind):
    """AWB on: the matrix carries no white balance (the gains are in the grid the loaders apply), the statistics come from
    the sources; two loads with an update in between, beside a twin without the options."""
    filt, pattern = FILTER_OF[kind], O.GBRG
    frames = [source(kind, SEAMS, 3 + k, levels=True) for k in range(2)]
    black, white, ccm = frames[0][2:5]
    wb = np.array([1.7, 1.0, 1.4])
    kw = dict(device=dev, correct_colors=True, color_correction=np.array(ccm), white_balance=wb, black_level=black,
              white_level=white, lens_shading=np.array(grid()), resize_width=RW, auto_white_balance=True, moving_alpha=0.5)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), **kw, **options(ti, "both", filt))
    twin = getattr(ti, cam)(ti.BayerPattern(pattern), **kw)
    got = capture(monkeypatch, isp)
    gains = []
    for k, f in enumerate(frames):
        what = f"{cam} {kind} load {k}"
        t = to_dev(f[0], dev)
        got.clear()
        img = call(isp, kind, t).cpu().numpy()
        call(twin, kind, t)
        pending = isp._awb_pending.cpu().numpy()
        assert pending.any()
        assert_exact(pending, twin._awb_pending.cpu().numpy(), what + ": the pending statistics")
        cfa = cfa_of(twin, f[1], work)                     # (the twin's grid: the user's with the current gains)
        if kind == "16u":
            assert len(got) == 2
            assert_exact(got[0].cpu().numpy(), got[1].cpu().numpy(), what + ": the twin's CFA")
            assert_exact(got[0].cpu().numpy(), cfa, what + " CFA")
        else:
            assert not got, "a packed frame without a map goes straight from the packed bytes"
        assert_exact(img, composed(cfa, pattern, ccm, work, "both", filt), what + " image (the matrix without the white balance)")
        with_wb = np.array(ccm) * wb[None, :]
        assert not np.array_equal(img, composed(cfa, pattern, with_wb, work, "both", filt)), "the white balance would show"
        gains.append(isp.white_balance_gains.cpu().numpy().copy())
        assert_exact(gains[-1], twin.white_balance_gains.cpu().numpy(), what + ": the gains")
        isp.update_white_balance(), twin.update_white_balance()
    assert_exact(gains[0], wb.astype(f32), "the seed")
    assert not np.array_equal(gains[1], gains[0]), "the update must move the gains"


@gpu
@pytest.mark.parametrize("cam,work", CAMS)
@pytest.mark.parametrize("kind", ["p12", "32f"])
def test_set_switches_the_options_between_two_loads(ti, dev, monkeypatch, cam, work, kind):
    """A CT sequence through one temporal history: the first load with the area resize, then set() turns the directional
    demosaic on and the resize to lanczos3."""
    H, W = SEAMS
    c = chain_case("CT", kind)
    st, mask, pattern = c["settings"], c["mask"], c["pattern"]
    m = the_map(H, W)
    kw = dict(device=dev, correct_colors=True, black_level=c["black"], white_level=c["white"], lens_shading=np.array(grid()),
              chromatic_aberration=st["C"], temporal_denoise=st["T"], resize_width=RW)
    isp = getattr(ti, cam)(ti.BayerPattern(pattern), resample=ti.Resample("area"), **kw)
    twin = getattr(ti, cam)(ti.BayerPattern(pattern), **kw)
    got, names = capture_both(monkeypatch, isp)
    hist, twin_hist = ti.TemporalHistory(), ti.TemporalHistory()
    for k, (step, opts, filt) in enumerate(zip(c["steps"], ("aa", "both"), ("area", "lanczos3"))):
        what = f"{cam} {kind} load {k} ({opts} {filt})"
        if k == 1:
            isp.set(demosaic=ti.Demosaic("directional"), resample=ti.Resample("lanczos3"))
            assert isp.demosaic == ti.Demosaic("directional") and isp.resample == ti.Resample("lanczos3")
        got.clear(), names.clear()
        src = to_dev(step["srcs"][0], dev)
        img = call(isp, kind, src, defects=m, history=hist).cpu().numpy()
        call(twin, kind, src, defects=m, history=twin_hist)
        assert names == ["_process_full" if kind in PACKED else "_process_image", "_process_image"] and len(got) == 2
        assert_exact(hist.plane.cpu().numpy(), twin_hist.plane.cpu().numpy(), what + ": the twin's history")
        assert_exact(hist.plane.cpu().numpy(), step["ys"]["T"], what + ": the temporal history")
        cfa = got[0].cpu().numpy()
        assert_exact(cfa, got[1].cpu().numpy(), what + ": the twin's CFA")
        assert_exact(cfa, cfa_of(isp, step["ys"]["T"], work, mask), what + " CFA")
        assert_exact(img, composed(cfa, pattern, isp.color_correct_matrix, work, opts, filt), what + " image")
    assert hist.frames == 2


@gpu
def test_process_packed12_with_both_options_and_highlights_is_the_two_calls(ti, dev):
    frames = [to_dev(source("p12", SEAMS, s)[0], dev) for s in range(3)]
    kw = dict(device=dev, moving_alpha=0.3, correct_colors=True, resize_width=RW, highlights=ti.Highlights("rebuild", 0.7),
              demosaic=ti.Demosaic("directional"), resample=ti.Resample("triangle"))
    a, b = ti.Camera16(ti.BayerPattern.RGGB, **kw), ti.Camera16(ti.BayerPattern.RGGB, **kw)
    for _ in range(2):
        outs = a.process_packed12(frames, gamma=0.8)
        want = b.tonemap_reinhard(b.load_packed12_batch(frames), gamma=0.8)
        for o, w in zip(outs, want):
            assert o.shape == (round(SEAMS[0] * RW / SEAMS[1]), RW, 3) and torch.equal(o, w)
        assert_exact(a.metrics.cpu().numpy(), b.metrics.cpu().numpy(), "metering")
    for off in ("demosaic", "resample", "highlights"):
        plain = ti.Camera16(ti.BayerPattern.RGGB, **{k: v for k, v in kw.items() if k != off})
        assert not torch.equal(plain.process_packed12(frames, gamma=0.8)[0], outs[0]), f"{off} must change the image"
